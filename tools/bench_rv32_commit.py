#!/usr/bin/env python3
"""What commit=True costs on one MI355X: one ELF that reads its input and commits what it read (a loop of RK_ECALL_READ
of 16 words, ALU work, RK_ECALL_COMMIT of 61 bytes from an odd address) proven through executor.execute_and_prove_p3
under chips="rv32im-mem", link=True, io=True with commit=False and commit=True, alternating in one process, at
shard_po2 16.  SP1's parameter set, every proof verified and the run chained inside.  One warm-up run of each route, then
--runs repetitions; one JSON line per run and one line of medians per route: milliseconds per verified shard of the
whole run (execution and setup included), trace cells per shard, the io and memop rows written per shard (active rows:
heads, word rows, commit-word rows; accesses) and the witness time per shard -- execute_rv32_device alone, the executor's
steps included, under a key set up before.

  python tools/bench_rv32_commit.py [--build LABEL] [--loops N] [--runs N] [--out FILE]"""
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
from raiko_amd.hal import HipHal, make_params  # noqa: E402

WORDS, BYTES = 16, 61


def committing_program(loops, spin=2000):
    """`loops` times: READ of 16 words, a spin loop of 3 `spin` cycles, loads of what arrived, COMMIT of 61 of its bytes
    from offset 1 (16 commit-word rows)"""
    p = A.li("s1", loops) + A.li("s0", BUF)
    p += ["outer:"] + _call(1, BUF, WORDS) + A.li("tp", spin)
    p += ["spin:", ("addi", "tp", "tp", -1), ("xor", "t2", "t2", "tp"), ("bne", "tp", "zero", "spin")]
    p += [("lw", "a2", 0, "s0"), ("lw", "a3", 60, "s0"), ("add", "s2", "s2", "a2")] + _call(2, BUF + 1, BYTES)
    p += [("addi", "s1", "s1", -1), ("bne", "s1", "zero", "outer")]
    return _elf(p + halt(0))


def witness_ms(hal, elf, words, params, commit):
    """execute_rv32_device alone -> (milliseconds per shard, io rows per shard, memop rows per shard: the heights)"""
    key = X.setup_rv32_elf(hal, elf, params, chips="rv32im-mem", link=True, io=True, commit=commit)
    try:
        hal.sync()
        t0 = time.perf_counter()
        out = X.execute_rv32_device(hal, elf, words, 16, chips="rv32im-mem", key=key, link=True, io=True, commit=commit)
        hal.sync()
        dt = time.perf_counter() - t0
        shards, bufs = out[1], out[3]
        n = len(shards)
        io_rows, memop_rows = (sum(1 << tables[i].log_height for tables, _ in shards) // n for i in (9, 7))
        for d in bufs:
            for b, _lg in d:
                b.free()
        return dt * 1e3 / n, io_rows, memop_rows
    finally:
        key.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="new")
    ap.add_argument("--loops", type=int, default=44)          # 6.0 k cycles a pass: 265 k cycles, 5 shards of 2^16
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    params = make_params(1)
    elf = committing_program(a.loops)
    words = [(0x9E3779B9 * (k + 1)) & 0xFFFFFFFF for k in range(WORDS * a.loops)]
    hal = HipHal(0)
    lines, per = [], {False: [], True: []}
    try:
        for run in range(-1, a.runs):                         # run -1 warms both routes up: module load, AIR compilation, allocator
            for commit in (False, True):
                t0 = time.perf_counter()
                ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=16, params=params, batch=3, chips="rv32im-mem",
                                                            link=True, io=True, commit=commit)
                dt = time.perf_counter() - t0
                wit, io_rows, memop_rows = witness_ms(hal, elf, words, params, commit)
                if run < 0:
                    continue
                assert len(ex.journal) == BYTES * a.loops
                cells = sum(t.air.width << t.log_height for tables, *_ in shards for t in tables)
                line = {"bench": "rv32_commit", "build": a.build, "run": run, "commit": commit, "shard_po2": 16, "cycles": ex.total_cycles,
                        "shards": len(proofs), "journal_bytes": len(ex.journal), "seconds": round(dt, 3),
                        "ms_per_shard": round(dt * 1e3 / len(proofs), 2), "trace_cells_per_shard": cells // len(proofs),
                        "io_rows_per_shard": io_rows, "memop_rows_per_shard": memop_rows, "witness_ms_per_shard": round(wit, 3)}
                if commit:
                    line["commit_word_rows_per_shard"] = sum(len(log) for log in ex.commit_logs) // len(proofs)
                per[commit].append(line)
                lines.append(line)
                print(json.dumps(line), flush=True)
    finally:
        hal.close()
    for commit in (False, True):
        if per[commit]:
            first = per[commit][0]
            med = {"bench": "rv32_commit", "build": a.build, "median_of": len(per[commit]), "commit": commit,
                   "ms_per_shard": statistics.median(r["ms_per_shard"] for r in per[commit]),
                   "witness_ms_per_shard": statistics.median(r["witness_ms_per_shard"] for r in per[commit]),
                   **{k: first[k] for k in ("trace_cells_per_shard", "io_rows_per_shard", "memop_rows_per_shard", "shards")}}
            lines.append(med)
            print(json.dumps(med), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()
