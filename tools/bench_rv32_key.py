#!/usr/bin/env python3
"""The rv32im-elf chip set next to rv32im on one MI355X: one ELF (tests/rv32_m_programs.py mixed_program, a long loop of
ALU work with M instructions among it) proven through executor.execute_and_prove_p3 under chips="rv32im" and
chips="rv32im-elf", alternating, three runs each, at shard_po2 16 and 20.  SP1's parameter set, every proof verified and
the run chained inside.  One JSON line per run: milliseconds per shard of the whole run (execution included; under
rv32im-elf the run includes the setup, reported on its own as well), the setup's time and the key's device bytes.

  python tools/bench_rv32_key.py [--build LABEL] [--chips rv32im,rv32im-elf] [--scale S] [--runs N]

--chips rv32im alone runs on a tree without the rv32im-elf chip set (the parent of the change that added it)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rv32_m_programs as MP  # noqa: E402
from raiko_amd import executor as X  # noqa: E402
from raiko_amd.hal import HipHal, make_params  # noqa: E402

INPUT = [1, 2, 3, 4]


def setup_cost(elf, params):
    """-> (milliseconds of setup_rv32_elf on a warm context, the key's device bytes)"""
    hal = HipHal(0)
    try:
        X.setup_rv32_elf(hal, elf, params).close()           # warm-up: module load, allocator
        t0 = time.perf_counter()
        key = X.setup_rv32_elf(hal, elf, params)
        ms = (time.perf_counter() - t0) * 1e3
        nbytes = key.bytes
        key.close()
        return ms, nbytes
    finally:
        hal.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="new")
    ap.add_argument("--chips", default="rv32im,rv32im-elf")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    routes = a.chips.split(",")
    params = make_params(1)
    elf = MP.mixed_program(int(44000 * a.scale))             # 74 instructions a pass: 3.26 M cycles, 4 shards of 2^20
    for chips in routes:                                     # warm-up of every route
        X.execute_and_prove_p3(MP.mixed_program(10), INPUT, shard_po2=13, params=params, batch=2, chips=chips)
    setup_ms = key_bytes = None
    if "rv32im-elf" in routes:
        setup_ms, key_bytes = setup_cost(elf, params)
    for po2 in (16, 20):
        for run in range(a.runs):
            for chips in routes:
                t0 = time.perf_counter()
                ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=po2, params=params, batch=3, chips=chips)
                dt = time.perf_counter() - t0
                cells = sum(t.air.width << t.log_height for tables, _ in shards for t in tables)
                line = {"bench": "rv32_key", "build": a.build, "run": run, "shard_po2": po2, "route": chips,
                        "cycles": ex.total_cycles, "shards": len(proofs), "seconds": round(dt, 3),
                        "ms_per_shard": round(dt * 1e3 / len(proofs), 2), "cycles_per_s": round(ex.total_cycles / dt),
                        "trace_cells_per_shard": cells // len(proofs)}
                if chips == "rv32im-elf":
                    line.update(setup_ms=round(setup_ms, 1), key_bytes=key_bytes)
                print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
