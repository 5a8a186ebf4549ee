#!/usr/bin/env python3
"""ELF -> verified shard proofs on one MI355X under the rv32i chip set (executor.execute_and_prove_p3(chips="rv32i"): the
five tables of every shard written on the GPU, every proof verified, the run chained by verify_rv32_execution) and the
rv32i-cf chip set (six tables, control flow and shifts constrained as well) next to the lookups-only route
(p3_trace_air(lookups=True)) on the same program, SP1's parameter set, 2^20-cycle shards; then both chip sets through
P3Pipeline (executor, table writing, proving and verification overlapped).  Prints one JSON line per
route: cycles/s and -- where the tables are at hand -- trace cells/s of the whole run (execution included)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rv32_chip_programs as RP  # noqa: E402
from raiko_amd import executor as X  # noqa: E402
from raiko_amd.hal import make_params  # noqa: E402


def main():
    loops = int(sys.argv[1]) if len(sys.argv) > 1 else 46000      # ~2.1 M cycles: two full shards and a partial one
    elf = RP.alu_program(loops)
    params = make_params(1)
    for chips in ("trace", "rv32i", "rv32i-cf"):
        t0 = time.perf_counter()
        if chips == "trace":
            ex, shards, proofs = X.execute_and_prove_p3(elf, [1, 2, 3, 4], shard_po2=20, params=params, batch=2, lookups=True)
        else:
            ex, shards, proofs = X.execute_and_prove_p3(elf, [1, 2, 3, 4], shard_po2=20, params=params, batch=2, chips=chips)
        dt = time.perf_counter() - t0
        cells = sum(t.air.width << t.log_height for tables, _ in shards for t in tables)
        print(json.dumps({"route": chips, "cycles": ex.total_cycles, "shards": len(proofs), "seconds": round(dt, 3),
                          "cycles_per_s": round(ex.total_cycles / dt), "trace_cells_per_s": round(cells / dt)}))
    for chips in ("rv32i", "rv32i-cf"):
        pipe = X.P3Pipeline(params, chips=chips)
        try:
            pipe.run(elf, [1, 2, 3, 4], shard_po2=20)            # warm-up: contexts, pools
            t0 = time.perf_counter()
            ex, proofs, _ = pipe.run(elf, [1, 2, 3, 4], shard_po2=20)
            dt = time.perf_counter() - t0
        finally:
            pipe.close()
        print(json.dumps({"route": chips + "-pipelined", "cycles": ex.total_cycles, "shards": len(proofs),
                          "seconds": round(dt, 3), "cycles_per_s": round(ex.total_cycles / dt)}))


if __name__ == "__main__":
    main()
