#!/usr/bin/env python3
"""The rv32im-mem chip set next to rv32im-elf on one MI355X: the same ELF proven through executor.execute_and_prove_p3
under chips="rv32im-elf" and chips="rv32im-mem", alternating, at shard_po2 16 and 20, on two guests:
tests/rv32_chip_programs.py alu_program (about one row in sixteen a load or a store, all at one word) and
tests/rv32_mem_programs.py loadstore_loop (all but two rows of its loop are loads and stores: memop is as tall as the
cpu table).  SP1's parameter set, every proof verified and the run chained inside.  One JSON line per run (milliseconds
per shard of the whole run, execution and setup included), then one summary line per (guest, shard_po2, route) with
minimum / median / maximum.

  python tools/bench_rv32_mem.py [--build LABEL] [--scale S] [--runs N] [--po2 16,20] [--guest NAME] [--witness]

--witness: time the witness generation alone instead (executor.execute_rv32_device: the executor and the shard tables
written on the GPU, no proofs): what the new kernels cost."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rv32_chip_programs as RP  # noqa: E402
import rv32_mem_programs as GP  # noqa: E402
from raiko_amd import executor as X  # noqa: E402
from raiko_amd.hal import HipHal, make_params  # noqa: E402

INPUT = [1, 2, 3, 4]
ROUTES = ("rv32im-elf", "rv32im-mem")


def witness_only(elf, po2, params, chips):
    hal = HipHal(0)
    try:
        key = X.setup_rv32_elf(hal, elf, params, chips=chips)
        try:
            t0 = time.perf_counter()
            ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, po2, chips=chips, key=key)
            hal.sync()
            dt = time.perf_counter() - t0
            for d in bufs:
                for b, _lg in d:
                    b.free()
            return ex, shards, dt
        finally:
            key.close()
    finally:
        hal.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build", default="new")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--po2", default="16,20")
    ap.add_argument("--guest", default="alu_program,loadstore_loop")
    ap.add_argument("--witness", action="store_true")
    a = ap.parse_args()
    params = make_params(1)
    # 47 and 66 cycles a pass: about 3.1 M cycles each, three shards of 2^20
    guests = {"alu_program": RP.alu_program(int(66000 * a.scale)), "loadstore_loop": GP.loadstore_loop(int(47000 * a.scale))}
    guests = {k: v for k, v in guests.items() if k in a.guest.split(",")}
    for chips in ROUTES:                                     # warm-up of every route
        if a.witness:
            witness_only(GP.loadstore_loop(10), 13, params, chips)
        else:
            X.execute_and_prove_p3(GP.loadstore_loop(10), INPUT, shard_po2=13, params=params, batch=2, chips=chips)
    seen = {}
    for guest, elf in guests.items():
        for po2 in [int(v) for v in a.po2.split(",")]:
            for run in range(a.runs):
                for chips in ROUTES:
                    if a.witness:
                        ex, shards, dt = witness_only(elf, po2, params, chips)
                    else:
                        t0 = time.perf_counter()
                        ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=po2, params=params, batch=3, chips=chips)
                        dt = time.perf_counter() - t0
                    n = len(shards)
                    cells = sum(t.air.width << t.log_height for tables, _ in shards for t in tables)
                    line = {"bench": "rv32_mem", "what": "witness" if a.witness else "prove", "build": a.build, "guest": guest, "run": run,
                            "shard_po2": po2, "route": chips, "cycles": ex.total_cycles, "shards": n, "seconds": round(dt, 3),
                            "ms_per_shard": round(dt * 1e3 / n, 2), "cycles_per_s": round(ex.total_cycles / dt),
                            "trace_cells_per_shard": cells // n, "log_heights_last_shard": [t.log_height for t in shards[-1][0]]}
                    print(json.dumps(line), flush=True)
                    seen.setdefault((guest, po2, chips), []).append(line["ms_per_shard"])
    for (guest, po2, chips), ms in seen.items():
        print(json.dumps({"bench": "rv32_mem", "what": "witness" if a.witness else "prove", "build": a.build, "summary": True, "guest": guest,
                          "shard_po2": po2, "route": chips, "runs": len(ms), "ms_per_shard_min": min(ms),
                          "ms_per_shard_median": round(statistics.median(ms), 2), "ms_per_shard_max": max(ms)}), flush=True)


if __name__ == "__main__":
    main()
