#!/usr/bin/env python3
"""The FRI query check of one shard proof with the Fiat-Shamir transcript proven too (raiko_amd/fri_transcript.py) beside
the statement without it (raiko_amd/fri_open.py), in one run on one MI355X under SP1's full parameter set:
  1. rk_p3_prove of a shard-shaped table (2^20 x 256 by default) -> shard proof
  2. the four captures (rk_p3_fri_openings, rk_p3_fri_inputs, rk_p3_fri_input_paths, rk_p3_fri_transcript) on the host
  3. per statement: the rows on the GPU (rk_fri_open_rows_device / rk_fri_transcript_rows_device), rk_p3_prove over the
     on_device tables, the statement verifier on the host
Two JSON lines, one per statement, appended to --out (profiles/fri_transcript_bench.jsonl); the second carries `added`:
what the transcript costs over the open statement in this run, and `chain`: the length of the challenger's chain.
  python tools/bench_fri_transcript.py [--shape 20x256] [--reps 3] [--out profiles/fri_transcript_bench.jsonl]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from raiko_amd import fri_open as O, fri_transcript as X, hal as H, p3  # noqa: E402


def measure(hal, mod, st, reps, verify):
    """(rows_ms, proof_ms, stage timing, proof, verify_ms, verdict) of one statement: best of `reps` after a warm-up"""
    for air in mod.airs(st):
        air.compile(hal)                                 # hiprtc, once per shape
    mod.device_tables(hal, st)
    rows_ms = None
    for _ in range(reps):
        t = time.perf_counter()
        d_tabs = mod.device_tables(hal, st)              # uploads publics and records, writes every table, waits
        ms = (time.perf_counter() - t) * 1e3
        rows_ms = ms if rows_ms is None else min(rows_ms, ms)
    mod.prove(hal, st, d_tabs)
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        proof = mod.prove(hal, st, d_tabs)
        ms = (time.perf_counter() - t) * 1e3
        if best is None or ms < best[0]:
            best = (ms, p3.last_timing(hal))
    t = time.perf_counter()
    rc = verify(proof)
    return rows_ms, best[0], best[1], proof, (time.perf_counter() - t) * 1e3, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="20x256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_transcript_bench.jsonl"))
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
    st = X.statement(tables, shard_proof, params=blob)
    extract_ms = (time.perf_counter() - t0) * 1e3
    lines, rc_all = [], 0
    for name, mod, s, verify in (("fri_open", O, st.opn, lambda pf: O.verify_open_statement(tables, shard_proof, (), pf, blob)),
                                 ("fri_transcript", X, st, lambda pf: X.verify_transcript_statement(tables, shard_proof, (), pf, blob))):
        sz = mod.sizes(s)
        rows_ms, proof_ms, stages, proof, verify_ms, rc = measure(hal, mod, s, args.reps, verify)
        rc_all |= rc
        lines.append({"statement": name, "shard": args.shape, "shape": dict(st.shape._asdict()), "shard_proof_words": int(shard_proof.size),
                      "matrices": len(st.opn.layout), "slots": len(st.opn.slots),
                      "rows": {n: sz[n + "_rows"] for n in mod.TABLE_NAMES},
                      "tables": {n: [1 << sz[n + "_log_height"], sz[n + "_width"]] for n in mod.TABLE_NAMES},
                      "rows_ms": round(rows_ms, 3), "proof_ms": round(proof_ms, 3),
                      "stages_ms": {a: round(b, 3) for a, b in stages.items()}, "proof_words": int(proof.size),
                      "verify_rc": rc, "verify_ms": round(verify_ms, 3)})
    lines[1]["extract_ms"] = round(extract_ms, 3)        # all four captures
    lines[1]["chain"] = {"permutations": len(st.plan.steps), "observed_words": int(st.observed.size), "sample_bits": st.plan.n_bits}
    lines[1]["added"] = {k: round(lines[1][k] - lines[0][k], 3) for k in ("rows_ms", "proof_ms", "verify_ms")}
    for line in lines:
        print(json.dumps(line), flush=True)
    if rc_all == 0 and args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hal.close()
    return 0 if rc_all == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
