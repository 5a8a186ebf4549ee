#!/usr/bin/env python3
"""ELF -> verified shard proofs on one MI355X under the rv32im chip set (executor.execute_and_prove_p3(chips="rv32im"):
the seven tables of every shard written on the GPU, every proof verified, the run chained) next to the rv32i-cf chip
set in the same run, on two programs: alu_program (tests/rv32_chip_programs.py: two M instructions in a loop of about
fifty) and an M-heavy loop (tests/rv32_m_programs.py m_program: nearly every row an M row).  SP1's parameter set,
2^20-cycle shards.  Prints one JSON line per route: cycles/s and trace cells/s of the whole run (execution included)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rv32_chip_programs as RP  # noqa: E402
import rv32_m_programs as MP  # noqa: E402
from raiko_amd import executor as X  # noqa: E402
from raiko_amd.hal import make_params  # noqa: E402


def main():
    scale = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    params = make_params(1)
    programs = (("alu_program", RP.alu_program(int(46000 * scale))), ("m_program", MP.m_program(int(2600 * scale))))
    X.execute_and_prove_p3(RP.alu_program(10), [1, 2, 3, 4], shard_po2=13, params=params, batch=2, chips="rv32im")  # warm-up
    for name, elf in programs:
        for chips in ("rv32i-cf", "rv32im"):
            t0 = time.perf_counter()
            ex, shards, proofs = X.execute_and_prove_p3(elf, [1, 2, 3, 4], shard_po2=20, params=params, batch=2, chips=chips)
            dt = time.perf_counter() - t0
            cells = sum(t.air.width << t.log_height for tables, _ in shards for t in tables)
            print(json.dumps({"program": name, "route": chips, "cycles": ex.total_cycles, "shards": len(proofs),
                              "seconds": round(dt, 3), "cycles_per_s": round(ex.total_cycles / dt),
                              "trace_cells_per_s": round(cells / dt)}), flush=True)


if __name__ == "__main__":
    main()
