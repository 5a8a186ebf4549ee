#!/usr/bin/env python3
"""Host time of rk_p3_verify and of the four captures that ride on it (rk_p3_fri_openings, rk_p3_fri_inputs,
rk_p3_fri_input_paths, rk_p3_fri_transcript) on the sp1_fib_k10_full proof (SP1's full parameter set: 100 queries, the
threaded path).  No GPU.  One build, or two against each other: with --libs every run is a fresh process per library,
the libraries taking turns, so that whatever else the machine does hits both alike.
  python tools/bench_p3_verify.py [--libs parent=old.so new=new.so] [--runs 21] [--out profiles/p3_verify_ab.jsonl]
One JSON line per run (lib, ms per call: the best of --reps calls in that process), then one summary line per library:
median, min and max over its runs."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CALLS = ("verify", "fri_openings", "fri_inputs", "fri_input_paths", "fri_transcript")


def one_run(reps):
    import oracle_lib as o
    from p3_cases import P3_CASES, init_of, tables_of
    from raiko_amd import fri_chip, fri_open, fri_reduce, fri_transcript, hal, p3
    case = "sp1_fib_k10_full"
    preset, over, _, _ = P3_CASES[case]
    o.oracle_set_params(preset, **over)
    blob = hal.make_params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf = o.oracle_p3_prove(tables, init)
    fns = {"verify": lambda: p3.verify(tables, pf, init, params=blob), "fri_openings": lambda: fri_chip.fri_openings(tables, pf, init, blob)[0],
           "fri_inputs": lambda: fri_reduce.fri_inputs(tables, pf, init, blob)[0], "fri_input_paths": lambda: fri_open.fri_input_paths(tables, pf, init, blob)[0],
           "fri_transcript": lambda: fri_transcript.fri_transcript(tables, pf, init, blob)[0]}
    ms = {}
    for name in CALLS:
        best = None
        for _ in range(reps + 1):                        # the first call warms up
            t = time.perf_counter()
            assert fns[name]() == 0
            d = (time.perf_counter() - t) * 1e3
            best = d if best is None else min(best, d)
        ms[name] = round(best, 3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="*", default=[])
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child or not args.libs:
        print(json.dumps(one_run(args.reps)), flush=True)
        return 0
    libs = dict(a.split("=", 1) for a in args.libs)           # name -> path
    lines, runs = [], {lib: [] for lib in libs}
    for i in range(args.runs):
        for lib, path in libs.items():
            env = dict(os.environ, RAIKO_HIP_LIB=os.path.abspath(path))
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], env=env, capture_output=True, text=True, check=True)
            ms = json.loads(out.stdout.strip().splitlines()[-1])
            runs[lib].append(ms)
            lines.append({"bench": "p3_verify_host", "lib": lib, "run": i, "ms": ms})
    for lib in libs:
        col = lambda c: [r[c] for r in runs[lib]]
        lines.append({"bench": "p3_verify_host", "lib": lib, "runs": args.runs,
                      "median_ms": {c: round(statistics.median(col(c)), 3) for c in CALLS},
                      "min_ms": {c: min(col(c)) for c in CALLS}, "max_ms": {c: max(col(c)) for c in CALLS}})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
