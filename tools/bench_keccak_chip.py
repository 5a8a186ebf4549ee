#!/usr/bin/env python3
"""The Keccak-f[1600] chip at the size of a block's hashing: 2^12 permutations = a 2^17-row table of 2537 columns under
SP1's full parameter set.  rk_keccak_chip_trace writes the rows on the GPU (timed alone: a host clock around the call and
a device synchronise; the write bandwidth it reaches = bytes written / time, beside HBM's nominal peak), rk_p3_prove
proves [claims, chip] over the device rows, rk_p3_verify checks.  One warm-up, then --reps repetitions; medians.
Appends one JSON line to profiles/keccak_chip_bench.jsonl.
  python tools/bench_keccak_chip.py [--log-perms 12] [--reps 5] [--out profiles/keccak_chip_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from raiko_amd import hal as H, keccak_chip as K, p3  # noqa: E402

HBM_PEAK_TBPS = 8.0              # MI355X HBM3E, nominal
README_G_CELLS_PER_S = 14.7      # README: a 2^20 x 256 table proven in 18.2 ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-perms", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keccak_chip_bench.jsonl"))
    args = ap.parse_args()
    from raiko_amd.hal import _ptr
    hal = H.HipHal(0)
    blob = hal.set_params(1)
    lib = H._lib.load()
    n = 1 << args.log_perms
    rows = K.min_rows(n)
    log_rows = rows.bit_length() - 1
    width = K.Layout.WIDTH
    states = np.random.default_rng(args.log_perms).integers(0, 1 << 64, size=(n, 25), dtype=np.uint64)
    d_in = hal.copy_from_elem(states.view(np.uint32).reshape(-1))
    d_rows, d_out = hal.alloc_elem(rows * width), hal.alloc_elem(n * 50)

    def write_rows():
        t0 = time.perf_counter()
        H._lib.check(hal._ctx, lib.rk_keccak_chip_trace(hal._ctx, _ptr(d_in), None, None, n, rows, _ptr(d_rows), _ptr(d_out)))
        hal.sync()
        return (time.perf_counter() - t0) * 1e3

    write_rows()
    trace_ms = statistics.median(write_rows() for _ in range(args.reps))
    outs = d_out.to_host().view(np.uint64).reshape(n, 25)
    chip_air = K.keccak_chip_air(blob)
    chip = p3.Table.pinned(chip_air, log_rows)
    claims = p3.Table.from_canonical(K.claims_air(int(blob.ext_w)), K.claims_rows(states, outs))
    tables, dev = [claims, chip], [None, (_ptr(d_rows), log_rows)]

    def prove():
        t0 = time.perf_counter()
        pf = p3.prove(hal, tables, device_traces=dev)
        return (time.perf_counter() - t0) * 1e3, pf, p3.last_timing(hal)

    prove()
    runs = [prove() for _ in range(args.reps)]
    prove_ms = statistics.median(r[0] for r in runs)
    mid = min(runs, key=lambda r: abs(r[0] - prove_ms))
    t0 = time.perf_counter()
    rc = p3.verify(tables, mid[1], params=blob)
    verify_ms = (time.perf_counter() - t0) * 1e3
    written = rows * width * 4 + n * 200
    cells = rows * (width + claims.trace.shape[1] * claims.trace.shape[0] / rows)
    info = chip_air.info()
    line = {"permutations": n, "rows": rows, "chip_columns": width, "reps": args.reps, "trace_ms_median": round(trace_ms, 4),
            "trace_bytes_written": written, "trace_write_TB_per_s": round(written / trace_ms / 1e9, 3), "hbm_nominal_peak_TB_per_s": HBM_PEAK_TBPS,
            "trace_permutations_per_s": round(n / trace_ms * 1e3, 1), "prove_ms_median": round(prove_ms, 3),
            "prove_ms_all": [round(r[0], 3) for r in runs], "stages_ms": {a: round(b, 3) for a, b in mid[2].items()},
            "trace_G_cells_per_s_proven": round(cells / prove_ms / 1e6, 3), "readme_G_cells_per_s_2_20_x_256": README_G_CELLS_PER_S,
            "permutations_proven_per_s": round(n / prove_ms * 1e3, 1), "ops_per_point": info["n_ops"], "fp_slots": info["n_fp_slots"],
            "constraints": info["n_constraints"], "proof_words": int(mid[1].size), "verify_rc": rc, "verify_ms": round(verify_ms, 2)}
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    hal.close()


if __name__ == "__main__":
    main()
