#!/usr/bin/env python3
"""What preprocessed columns buy: one cpu-like table (2^log_cpu x width, degree 3) with `lookups` range lookups into a
2^log_range-row range table, proven twice in one run on one build --
  (a) main:  the range values in the main trace, the range AIR with its counter constraints (lookup_demo_airs' form)
  (b) prep:  the range values preprocessed (p3_range_air_prep), the key made once OUTSIDE the timed region
alternating a, b, a, b ..: rk_p3_last_timing per stage of every repetition, their medians, rk_p3_setup's time and the
key's bytes.  Both proofs are verified.
  python tools/bench_p3_prep.py [--log-cpu 20] [--width 256] [--lookups 16] [--log-range 16] [--reps 5] [--jit]
Prints one JSON line (profiles/p3_prep_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from raiko_amd import hal as H, p3  # noqa: E402


def cpu_air(width, lookups, seed=7):
    """p3.local_air's shape -- inputs in the first half (column 0 counts rows), column half + k = in_i in_j in_l + in_m --
    whose input columns 1 .. lookups are sent on the RANGE bus, once per row each"""
    half = width // 2
    assert 1 + lookups <= half
    rng = np.random.default_rng(seed)
    b = p3.AirBuilder(width, 0)
    b.when_first_row().assert_zero(b.local(0))
    b.when_transition().assert_eq(b.next(0), b.local(0) + 1)
    picks = rng.integers(0, half, size=(half, 4))
    for k in range(half):
        i, j, l, m = (int(v) for v in picks[k])
        b.assert_eq(b.local(half + k), b.local(i) * b.local(j) * b.local(l) + b.local(m))
    for c in range(1, 1 + lookups):
        b.send(p3.BUS_RANGE, [c])
    air = b.build()
    air.picks = picks
    return air


def device_traces(torch, air, log_n, lookups, log_range, seed):
    """the cpu trace on the GPU (Montgomery words, int32 view) and the multiplicity of every range value"""
    P = p3.P
    n, w = 1 << log_n, air.width
    half = w // 2
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    c = torch.zeros((w, n), dtype=torch.int64, device="cuda")
    c[:half] = torch.randint(0, P, (half, n), dtype=torch.int64, device="cuda", generator=g)
    c[0] = torch.arange(n, dtype=torch.int64, device="cuda") % P
    c[1:1 + lookups] = torch.randint(0, 1 << log_range, (lookups, n), dtype=torch.int64, device="cuda", generator=g)
    for k in range(half):
        i, j, l, m = (int(v) for v in air.picks[k])
        c[half + k] = (c[i] * c[j] % P * c[l] + c[m]) % P
    counts = torch.bincount(c[1:1 + lookups].reshape(-1), minlength=1 << log_range)
    mont = c * ((1 << 32) % P) % P
    return mont.t().contiguous().to(torch.int32), counts.cpu().numpy().astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-cpu", type=int, default=20)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--lookups", type=int, default=16)
    ap.add_argument("--log-range", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--jit", action="store_true")
    args = ap.parse_args()
    import torch
    hal = H.HipHal(0)
    blob = hal.set_params(1)
    air = cpu_air(args.width, args.lookups)
    cpu_dev, counts = device_traces(torch, air, args.log_cpu, args.lookups, args.log_range, 8)
    values = np.arange(1 << args.log_range, dtype=np.uint64)
    rng_main = p3.Table.from_canonical(p3.lookup_demo_airs()[3], np.stack([values, counts % p3.P], axis=1))
    rng_prep = p3.Table.from_canonical(p3.p3_range_air_prep(), (counts % p3.P).reshape(-1, 1), (), prep=values.reshape(-1, 1))
    cpu = p3.Table(air, None, [])
    cpu.log_height = args.log_cpu
    if args.jit:
        for a in (air, rng_main.air, rng_prep.air):
            a.compile(hal)
    dev = [(cpu_dev.data_ptr(), args.log_cpu), None]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    key = p3.setup(hal, [cpu, rng_prep])
    setup_ms = (time.perf_counter() - t0) * 1e3          # rk_p3_setup synchronises before it returns
    variants = {"main": ([cpu, rng_main], None), "prep": ([cpu, rng_prep], key)}
    proofs = {}
    for name, (tables, k) in variants.items():            # warm-up: first-touch allocations, code objects
        proofs[name] = p3.prove(hal, tables, device_traces=dev, key=k)
    runs = {name: [] for name in variants}
    for _ in range(args.reps):
        for name, (tables, k) in variants.items():
            t1 = time.perf_counter()
            p3.prove(hal, tables, device_traces=dev, key=k)
            wall = (time.perf_counter() - t1) * 1e3
            runs[name].append(dict(p3.last_timing(hal), wall=wall))
    out = {"log_cpu": args.log_cpu, "width": args.width, "lookups": args.lookups, "log_range": args.log_range, "jit": args.jit, "reps": args.reps,
           "setup_ms": round(setup_ms, 3), "key_bytes": key.bytes}
    for name in variants:
        out[name] = {"median_ms": {s: round(statistics.median(r[s] for r in runs[name]), 3) for s in runs[name][0]},
                     "total_ms_runs": [round(r["total"], 3) for r in runs[name]], "proof_words": int(proofs[name].size)}
    out["main"]["verify_rc"] = p3.verify([cpu, rng_main], proofs["main"], params=blob)
    out["prep"]["verify_rc"] = p3.verify([cpu, p3_pinned(rng_prep)], proofs["prep"], params=blob, prep_root=key.root)
    key.close()
    hal.close()
    print(json.dumps(out), flush=True)


def p3_pinned(t):
    v = p3.Table(t.air, None, t.public_values)
    v.log_height = t.log_height
    return v


if __name__ == "__main__":
    main()
