#!/usr/bin/env python3
"""The link between shard memories next to the unlinked rv32im-mem chip set on one MI355X: one ELF
(tests/rv32_mem_programs.py loadstore_loop: every row but two a load or a store) proven through
executor.execute_and_prove_p3(chips="rv32im-mem") with link=True and link=False in the same process, alternating, five
repetitions each, at 2^16-cycle shards.  SP1's parameter set, every proof verified inside (with its claims under the
link) and the run chained.  The yardstick is the link=False run of the same call.  JSON lines:

  run       one per repetition and route: seconds, milliseconds per verified shard, touched words per shard
  summary   the medians of both routes, their ratio, and the spread of the link=False repetitions among themselves
  journal   rk_rv32mem_journal_device alone on one shard's finished memory table (kernel, commitment, read-back)
  verify    host time of verify_rv32_shard on one shard: with its journal (digest, claims) and, on the unlinked proof,
            without
  digest    rk_rv32mem_journal_root on the host at the largest journal a 2^16 shard admits: 2^17 rows

  python tools/bench_rv32_link.py [--build LABEL] [--loops N] [--runs N]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rv32_mem_programs as GP  # noqa: E402
from raiko_amd import executor as X  # noqa: E402
from raiko_amd import p3, rv32_sets, rv32link, rv32mem  # noqa: E402
from raiko_amd.hal import HipHal, make_params  # noqa: E402

INPUT = [1, 2, 3, 4]
PO2 = 16


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="new")
    ap.add_argument("--loops", type=int, default=4000)       # 66 instructions a pass: 264 k cycles, 5 shards of 2^16
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    params = make_params(1)
    elf = GP.loadstore_loop(a.loops)
    say = lambda **kw: print(json.dumps(dict(bench="rv32_link", build=a.build, **kw)), flush=True)
    for link in (False, True):                               # warm-up of both routes
        X.execute_and_prove_p3(GP.loadstore_loop(10), INPUT, shard_po2=13, params=params, batch=2, chips="rv32im-mem", link=link)
    ms, kept = {False: [], True: []}, {}
    for run in range(a.runs):
        for link in (False, True):
            t0 = time.perf_counter()
            ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=PO2, params=params, batch=3, chips="rv32im-mem", link=link)
            dt = time.perf_counter() - t0
            ms[link].append(dt * 1e3 / len(proofs))
            kept[link] = (ex, shards, proofs)
            words = [int(p[1 + 8]) for p in proofs]          # the memory table's log height, as the proof carries it
            say(kind="run", run=run, link=link, shard_po2=PO2, cycles=ex.total_cycles, shards=len(proofs), seconds=round(dt, 3),
                ms_per_shard=round(ms[link][-1], 2), memory_log_rows=words,
                touched_words_per_shard=[len(j) for j in ex.journals] if link else None)
    med = {k: statistics.median(v) for k, v in ms.items()}
    say(kind="summary", shard_po2=PO2, runs=a.runs, ms_per_shard_unlinked=round(med[False], 2), ms_per_shard_linked=round(med[True], 2),
        linked_over_unlinked=round(med[True] / med[False], 4),
        unlinked_spread=round((max(ms[False]) - min(ms[False])) / med[False], 4), linked_spread=round((max(ms[True]) - min(ms[True])) / med[True], 4))
    # rk_rv32mem_journal_device alone, on the memory table of the first shard and on the tallest a 2^16 shard admits
    ref = X.execute(elf, INPUT, segment_limit_po2=PO2, record_trace=True)
    hal = HipHal(0)
    try:
        hal.set_params(1)
        tall = np.zeros((1 << (PO2 + 1), rv32mem.MEMORY_COLS), dtype=np.int64)
        tall[:, rv32mem.B_WL], tall[:, rv32mem.B_WH] = np.arange(1 << 17) & 0x3FFF, np.arange(1 << 17) >> 14
        tall[:, rv32mem.B_I_LO], tall[:, rv32mem.B_F_HI], tall[:, rv32mem.B_REAL] = 7, 9, 1
        for what, table in (("first shard", rv32mem.memory_rows(ref.mem[0])[0]), ("2^17 real rows", tall)):
            buf = hal.copy_from_elem(np.ascontiguousarray(p3.to_mont(table)).reshape(-1))
            hal.sync()
            lg = table.shape[0].bit_length() - 1
            try:
                rv32_sets.journal_device(hal, buf, lg)       # warm-up
                say(kind="journal", what=what, memory_rows=table.shape[0], real_rows=int(table[:, rv32mem.B_REAL].sum()),
                    ms=round(timed(lambda: rv32_sets.journal_device(hal, buf, lg), 9), 3))
            finally:
                buf.free()
    finally:
        hal.close()
    # the verifier's host time on one shard
    for link in (False, True):
        ex, shards, proofs = kept[link]
        vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height)
        tables, init = shards[0][:2]
        jk = dict(journal=ex.journals[0]) if link else {}
        assert X.verify_rv32_shard(tables, proofs[0], init, params, **vk, **jk) == 0
        say(kind="verify", link=link, touched_words=len(ex.journals[0]) if link else None,
            ms=round(timed(lambda: X.verify_rv32_shard(tables, proofs[0], init, params, **vk, **jk), 9), 3))
    # the host digest of the largest journal a 2^16 shard admits
    big = np.stack([np.arange(1 << 17, dtype=np.uint32) * 3, np.full(1 << 17, 0x01020304, dtype=np.uint32),
                    np.arange(1 << 17, dtype=np.uint32)], axis=1)
    say(kind="digest", rows=1 << 17, log_rows=17, ms=round(timed(lambda: rv32link.journal_root(big, 17, params), 5), 2))
    claims = rv32link.claims_of(big)
    say(kind="claims_of", rows=1 << 17, ms=round(timed(lambda: rv32link.claims_of(big), 3), 2), tuples=int(claims[0][2].shape[0]))
    fresh = big.copy()
    fresh[:, 1] = 0                                          # words outside the image start from zero
    say(kind="replay", rows=1 << 17, ms=round(timed(lambda: rv32link.check_memory_chain([fresh], {}), 3), 2))


if __name__ == "__main__":
    main()
