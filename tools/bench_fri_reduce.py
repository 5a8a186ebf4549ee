#!/usr/bin/env python3
"""The FRI query check of one shard proof from the opened rows on -- reduced openings and commit phase as lookup tables
(raiko_amd/fri_reduce.py) --, end to end on one MI355X under SP1's full parameter set:
  1. rk_p3_prove of a shard-shaped table (2^20 x 256 by default) -> shard proof
  2. rk_p3_fri_openings + rk_p3_fri_inputs: the verdict, layout, public values and per-query records (host)
  3. rk_fri_reduce_rows_device: the fold', path, reduce and Poseidon2 chip rows (GPU; they stay in HBM)
  4. rk_p3_prove over the four on_device tables -> the proof
  5. verify_reduce_statement (host): shape, layout and public values recomputed from the shard proof, heights pinned,
     proof verified
One JSON line, appended to --out (profiles/fri_reduce_bench.jsonl).  tools/bench_fri_chip.py measures the smaller statement
(the commit phase alone) on the same shard proof: the difference is what the reduced openings cost.
  python tools/bench_fri_reduce.py [--shape 20x256] [--reps 3] [--out profiles/fri_reduce_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from raiko_amd import fri_reduce as G, hal as H, p3  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="20x256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_reduce_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import bench_p3
    hal = H.HipHal(0)
    blob = hal.set_params(1)
    tables, bufs, dev = [], [], []
    for i, spec in enumerate(args.shape.split(",")):
        k, w = (int(v) for v in spec.split("x"))
        air = p3.local_air(w, seed=7 + i)
        air.compile(hal)
        t = p3.Table(air, None, [])
        t.log_height = k
        tables.append(t)
        b = bench_p3.device_trace(torch, air, k, 8 + i)
        bufs.append(b)
        dev.append((b.data_ptr(), k))
    torch.cuda.synchronize()
    shard_proof = p3.prove(hal, tables, device_traces=dev)
    t0 = time.perf_counter()
    st = G.statement(tables, shard_proof, params=blob)
    extract_ms = (time.perf_counter() - t0) * 1e3
    sz = G.sizes(st)
    for air in G.airs(st):
        air.compile(hal)                                 # hiprtc, once per shape
    G.device_tables(hal, st)
    rows_ms = None
    for _ in range(args.reps):
        t1 = time.perf_counter()
        d_tabs = G.device_tables(hal, st)                # uploads publics and records, writes all four tables, waits
        ms = (time.perf_counter() - t1) * 1e3
        rows_ms = ms if rows_ms is None else min(rows_ms, ms)
    G.prove(hal, st, d_tabs)
    best = None
    for _ in range(args.reps):
        t2 = time.perf_counter()
        proof = G.prove(hal, st, d_tabs)
        ms = (time.perf_counter() - t2) * 1e3
        if best is None or ms < best[0]:
            best = (ms, p3.last_timing(hal))
    t3 = time.perf_counter()
    rc = G.verify_reduce_statement(tables, shard_proof, (), proof, blob)
    verify_ms = (time.perf_counter() - t3) * 1e3
    line = {"shard": args.shape, "shape": dict(st.shape._asdict()), "shard_proof_words": int(shard_proof.size),
            "matrices": len(st.layout), "slots": len(st.slots),
            "rows": {n: sz[n + "_rows"] for n in G.TABLE_NAMES},
            "tables": {n: [1 << sz[n + "_log_height"], sz[n + "_width"]] for n in G.TABLE_NAMES},
            "extract_ms": round(extract_ms, 3), "rows_ms": round(rows_ms, 3), "proof_ms": round(best[0], 3),
            "stages_ms": {a: round(b, 3) for a, b in best[1].items()}, "proof_words": int(proof.size),
            "verify_rc": rc, "verify_ms": round(verify_ms, 3)}
    print(json.dumps(line), flush=True)
    if rc == 0 and args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    hal.close()
    return 0 if rc == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
