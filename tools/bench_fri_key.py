#!/usr/bin/env python3
"""The transcript statement (raiko_amd/fri_transcript.py) over an rv32im-elf shard proof -- a proof under a verifying key,
four input batches -- beside the same statement over the rv32im proof of the same ELF and shard, in one run on one MI355X
under SP1's full parameter set:
  1. execute_and_prove_p3 of one ELF (tests/rv32_m_programs.py mixed_program) under both chip sets; the first shard's proof
  2. the four captures on the host (the _key ones with ex.prep_root for rv32im-elf)
  3. per variant: the rows on the GPU (rk_fri_transcript_rows_device), rk_p3_prove over the on_device tables, the
     statement verifier on the host (bound to ex.prep_root for rv32im-elf)
One warm-up of every timed call, then --reps repetitions with the two variants ALTERNATING; every line reports the
minimum, the median and the maximum over them.  One JSON line per variant, appended to --out
(profiles/fri_key_bench.jsonl), with the rows written per table; the rv32im-elf line carries `reduce_rows_vs_rv32im`.
  python tools/bench_fri_key.py [--shard-po2 16] [--loops 800] [--reps 5] [--out profiles/fri_key_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rv32_m_programs as MP  # noqa: E402
from raiko_amd import executor as E, fri_transcript as X, hal as H, p3  # noqa: E402

INPUT = [1, 2, 3, 4]


def spread(ms):
    return {"min": round(min(ms), 3), "median": round(statistics.median(ms), 3), "max": round(max(ms), 3), "n": len(ms)}


def timed(fn):
    t = time.perf_counter()
    out = fn()                                           # every call below ends in a device synchronise or is host code
    return (time.perf_counter() - t) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shard-po2", type=int, default=16)
    ap.add_argument("--loops", type=int, default=800)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fri_key_bench.jsonl"))
    a = ap.parse_args()
    params = H.make_params(1)
    elf = MP.mixed_program(a.loops)
    variants = {}
    for chips in ("rv32im", "rv32im-elf"):
        ex, shards, proofs = E.execute_and_prove_p3(elf, INPUT, shard_po2=a.shard_po2, params=params, chips=chips)
        tables, init = shards[0]
        root = getattr(ex, "prep_root", None) if chips == "rv32im-elf" else None
        ver = E.rv32_verifier_tables(tables, proofs[0], root, getattr(ex, "program_log_height", None) if root is not None else None)
        variants[chips] = dict(ver=ver, init=init, pf=proofs[0], root=root, shards=len(proofs),
                               trace_cells=sum(t.air.width << t.log_height for t in tables),
                               prep_cells=sum(t.air.prep_width << t.log_height for t in tables))
    hal = H.HipHal(0)
    blob = hal.set_params(1)
    times = {c: {"extract_ms": [], "rows_ms": [], "proof_ms": [], "verify_ms": []} for c in variants}
    for c, v in variants.items():                        # statements, hiprtc once per shape, one warm-up of every timed call
        v["st"] = X.statement(v["ver"], v["pf"], v["init"], blob, prep_root=v["root"])
        for air in X.airs(v["st"]):
            air.compile(hal)
        v["dev"] = X.device_tables(hal, v["st"])
        v["proof"] = X.prove(hal, v["st"], v["dev"])
        v["rc"] = X.verify_transcript_statement(v["ver"], v["pf"], v["init"], v["proof"], blob, prep_root=v["root"])
    for _ in range(a.reps):
        for c, v in variants.items():
            t = times[c]
            t["extract_ms"].append(timed(lambda: X.statement(v["ver"], v["pf"], v["init"], blob, prep_root=v["root"]))[0])
            ms, v["dev"] = timed(lambda: X.device_tables(hal, v["st"]))
            t["rows_ms"].append(ms)
            ms, proof = timed(lambda: X.prove(hal, v["st"], v["dev"]))
            t["proof_ms"].append(ms)
            assert (proof == v["proof"]).all()
            ms, rc = timed(lambda: X.verify_transcript_statement(v["ver"], v["pf"], v["init"], proof, blob, prep_root=v["root"]))
            t["verify_ms"].append(ms)
            v["rc"] |= rc
    lines, rc_all = [], 0
    for c, v in variants.items():
        st, sz = v["st"], X.sizes(v["st"])
        rc_all |= v["rc"]
        lines.append({"bench": "fri_key", "statement": "fri_transcript", "chips": c, "keyed": v["root"] is not None, "shard_po2": a.shard_po2,
                      "shards": v["shards"], "shape": dict(st.shape._asdict()), "shard_proof_words": int(v["pf"].size),
                      "shard_trace_cells": v["trace_cells"], "shard_prep_cells": v["prep_cells"],
                      "matrices": len(st.opn.layout), "slots": len(st.opn.slots), "batches": sz["n_batches"],
                      "log_pmax": sz["log_pmax"], "log_kmax": sz["log_kmax"],
                      "rows": {n: sz[n + "_rows"] for n in X.TABLE_NAMES}, "rows_total": sum(sz[n + "_rows"] for n in X.TABLE_NAMES),
                      "tables": {n: [1 << sz[n + "_log_height"], sz[n + "_width"]] for n in X.TABLE_NAMES},
                      "extract_ms": spread(times[c]["extract_ms"]), "rows_ms": spread(times[c]["rows_ms"]),
                      "proof_ms": spread(times[c]["proof_ms"]), "verify_ms": spread(times[c]["verify_ms"]),
                      "proof_words": int(v["proof"].size), "verify_rc": v["rc"]})
    lines[1]["reduce_rows_vs_rv32im"] = round(lines[1]["rows"]["reduce"] / lines[0]["rows"]["reduce"], 4)
    for line in lines:
        print(json.dumps(line), flush=True)
    if rc_all == 0 and a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    hal.close()
    return 0 if rc_all == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
