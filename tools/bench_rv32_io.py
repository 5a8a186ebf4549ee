#!/usr/bin/env python3
"""What io=True costs on one MI355X: one ELF that reads its input (a loop of RK_ECALL_READ of 16 words and ALU work
between the calls) proven through executor.execute_and_prove_p3 under chips="rv32im-mem", link=True with io=False and
io=True, alternating in one process, at shard_po2 16.  SP1's parameter set, every proof verified and the run chained
inside.  One warm-up run of each route, then --runs repetitions; one JSON line per run and one line of medians per
route: milliseconds per verified shard of the whole run (execution and setup included), trace cells per shard, and --
io=True -- the verifier's host time for the input digests (rk_rv32mem_journal_root over every shard's slice), per shard.

  python tools/bench_rv32_io.py [--build LABEL] [--loops N] [--runs N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rv32_asm as A  # noqa: E402
from rv32_io_programs import BUF, _call, halt  # noqa: E402
from rv32_mem_programs import _elf  # noqa: E402
from raiko_amd import executor as X  # noqa: E402
from raiko_amd import rv32io  # noqa: E402
from raiko_amd.hal import make_params  # noqa: E402

WORDS = 16


def reading_program(loops, spin=2000):
    """`loops` times: READ of 16 words, a spin loop of 3 `spin` cycles, loads of what arrived"""
    p = A.li("s1", loops) + A.li("s0", BUF)
    p += ["outer:"] + _call(1, BUF, WORDS) + A.li("tp", spin)
    p += ["spin:", ("addi", "tp", "tp", -1), ("xor", "t2", "t2", "tp"), ("bne", "tp", "zero", "spin")]
    p += [("lw", "a2", 0, "s0"), ("lw", "a3", 60, "s0"), ("add", "s2", "s2", "a2"), ("addi", "s1", "s1", -1), ("bne", "s1", "zero", "outer")]
    return _elf(p + halt(0))


def digest_ms(shards, words, params):
    """the verifier's host time for the input digests of a run, milliseconds"""
    t0 = time.perf_counter()
    for tables, _init in shards:
        io = tables[rv32io.IO_TABLE]
        pub = rv32io.publics_of(io.public_values)
        rv32io.stream_root(pub["pos_start"], words[pub["pos_start"]:pub["pos_end"]], io.log_height, params)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="new")
    ap.add_argument("--loops", type=int, default=44)          # 6.0 k cycles a pass: 265 k cycles, 5 shards of 2^16
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    params = make_params(1)
    elf = reading_program(a.loops)
    words = [(0x9E3779B9 * (k + 1)) & 0xFFFFFFFF for k in range(WORDS * a.loops)]
    lines, per = [], {False: [], True: []}
    for run in range(-1, a.runs):                             # run -1 warms both routes up: module load, AIR compilation, allocator
        for io in (False, True):
            t0 = time.perf_counter()
            ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=16, params=params, batch=3, chips="rv32im-mem", link=True, io=io)
            dt = time.perf_counter() - t0
            if run < 0:
                continue
            cells = sum(t.air.width << t.log_height for tables, _ in shards for t in tables)
            line = {"bench": "rv32_io", "build": a.build, "run": run, "io": io, "shard_po2": 16, "cycles": ex.total_cycles,
                    "shards": len(proofs), "input_words": ex.input_words_read, "seconds": round(dt, 3),
                    "ms_per_shard": round(dt * 1e3 / len(proofs), 2), "trace_cells_per_shard": cells // len(proofs)}
            if io:
                line["verifier_digest_ms_per_shard"] = round(digest_ms(shards, words, params) / len(proofs), 3)
            per[io].append(line)
            lines.append(line)
            print(json.dumps(line), flush=True)
    for io in (False, True):
        if per[io]:
            med = {"bench": "rv32_io", "build": a.build, "median_of": len(per[io]), "io": io,
                   "ms_per_shard": statistics.median(r["ms_per_shard"] for r in per[io]),
                   "trace_cells_per_shard": per[io][0]["trace_cells_per_shard"], "shards": per[io][0]["shards"]}
            if io:
                med["verifier_digest_ms_per_shard"] = statistics.median(r["verifier_digest_ms_per_shard"] for r in per[io])
            lines.append(med)
            print(json.dumps(med), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
