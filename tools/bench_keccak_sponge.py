#!/usr/bin/env python3
"""The Keccak-256 sponge table at the size of a block's hashing: 2^12 blocks under SP1's full parameter set, as three
distributions -- 4096 one-block messages, 64 messages of 64 blocks, one message of 4096 blocks.  The chain of a
message's permutations is dependent, so the distributions differ in the states kernel and in nothing else.

Per distribution: rk_keccak_sponge_trace (both kernels; a host clock around the call and a device synchronise),
rk_keccak_chip_trace from the states buffer on the device, rk_p3_prove of [sponge, chip] over the device rows with
`statement`'s init words, verify_keccak256.  One warm-up of every shape, then --reps repetitions that ALTERNATE between the
distributions; medians.  The split of the trace call into its two kernels comes from a profiler run of its own:
  rocprofv3 --kernel-trace --stats -f csv -d DIR/<dist> -o ks -- python tools/bench_keccak_sponge.py --kernels-only --dist <dist>
for <dist> in 4096x1 64x64 1x4096, then --kernel-stats DIR on the timed run (without it the split is null: not measured).
Appends one JSON line per distribution to profiles/keccak_sponge_bench.jsonl.
  python tools/bench_keccak_sponge.py [--log-blocks 12] [--reps 5] [--kernel-stats DIR] [--out profiles/keccak_sponge_bench.jsonl]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from raiko_amd import hal as H, keccak, keccak_chip as K, keccak_sponge as S, p3  # noqa: E402

HBM_PEAK_TBPS = 8.0              # MI355X HBM3E, nominal
PARENT = {"chip_rows_ms": 0.294, "chip_rows_TB_per_s": 4.52, "prove_claims_chip_ms": 69.5,           # profiles/keccak_chip_bench.jsonl
          "p2_chain_us_per_permutation_half_wave": 2.7, "p2_chain_us_per_permutation_lane_per_chain": 18.0}


def distributions(log_blocks):
    n = 1 << log_blocks
    side = 1 << (log_blocks // 2)
    return {"%dx1" % n: (n, 1), "%dx%d" % (side, n // side): (side, n // side), "1x%d" % n: (1, n)}


def messages(n_msgs, blocks_each, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=136 * (blocks_each - 1) + 50, dtype=np.uint8).tobytes() for _ in range(n_msgs)]


def kernel_split(stats_dir, dist):
    """{kernel: (calls, average ns, min ns)} of the two sponge kernels from rocprofv3's kernel stats of one distribution"""
    out = {}
    for path in glob.glob(os.path.join(stats_dir, dist, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for k in ("keccak_sponge_chain_kernel", "keccak_sponge_rows_kernel"):
                    if k in row["Name"]:
                        out[k] = (int(row["Calls"]), float(row["AverageNs"]), float(row["MinNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-blocks", type=int, default=12)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dist", default=None, help="one distribution only")
    ap.add_argument("--kernels-only", action="store_true", help="the trace calls alone: what a profiler run wraps")
    ap.add_argument("--kernel-stats", default=None, help="directory of rocprofv3 kernel stats, one subdirectory a distribution")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keccak_sponge_bench.jsonl"))
    args = ap.parse_args()
    from raiko_amd.hal import _ptr
    hal = H.HipHal(0)
    blob = hal.set_params(1)
    lib = H._lib.load()
    dists = distributions(args.log_blocks)
    if args.dist is not None:
        dists = {args.dist: dists[args.dist]}
    nb = 1 << args.log_blocks
    rows, chip_rows = S.min_rows(nb), K.min_rows(nb)
    width, chip_width = S.Layout.WIDTH, K.Layout.WIDTH
    sponge_air, chip_air = S.keccak_sponge_air(blob), K.keccak_chip_air(blob)

    class Case:
        pass

    cases = {}
    for i, (name, (k, each)) in enumerate(dists.items()):
        c = Case()
        c.msgs = messages(k, each, 100 + i)
        blocks, first = S.pad_blocks(c.msgs)
        assert blocks.shape[0] == nb and len(first) == k + 1
        c.k = k
        c.d_blocks, c.d_first = hal.copy_from_elem(blocks.view(np.uint32).reshape(-1)), hal.copy_from_elem(first)
        c.d_rows, c.d_states, c.d_outs, c.d_dig = hal.alloc_elem(rows * width), hal.alloc_elem(nb * 50), hal.alloc_elem(nb * 50), hal.alloc_elem(k * 8)
        c.trace_ms, c.chip_ms, c.prove = [], [], []
        cases[name] = c

    def write_rows(c):
        t0 = time.perf_counter()
        H._lib.check(hal._ctx, lib.rk_keccak_sponge_trace(hal._ctx, _ptr(c.d_blocks), _ptr(c.d_first), None, c.k, nb, rows, _ptr(c.d_rows),
                                                          _ptr(c.d_states), _ptr(c.d_outs), _ptr(c.d_dig)))
        hal.sync()
        return (time.perf_counter() - t0) * 1e3

    for c in cases.values():
        write_rows(c)
    for _ in range(args.reps):
        for c in cases.values():
            c.trace_ms.append(write_rows(c))
    if args.kernels_only:
        print(json.dumps({n: round(statistics.median(c.trace_ms), 4) for n, c in cases.items()}))
        hal.close()
        return

    d_chip = hal.alloc_elem(chip_rows * chip_width)

    def write_chip(c):
        t0 = time.perf_counter()
        H._lib.check(hal._ctx, lib.rk_keccak_chip_trace(hal._ctx, _ptr(c.d_states), None, None, nb, chip_rows, _ptr(d_chip), None))
        hal.sync()
        return (time.perf_counter() - t0) * 1e3

    tables = [p3.Table.pinned(sponge_air, rows.bit_length() - 1), p3.Table.pinned(chip_air, chip_rows.bit_length() - 1)]

    def prove(c):
        write_chip(c)                   # one chip buffer: its rows are this distribution's again
        dev = [(_ptr(c.d_rows), rows.bit_length() - 1), (_ptr(d_chip), chip_rows.bit_length() - 1)]
        t0 = time.perf_counter()
        pf = p3.prove(hal, tables, c.init, device_traces=dev)
        return (time.perf_counter() - t0) * 1e3, pf, p3.last_timing(hal)

    for c in cases.values():
        c.digests = S.digest_bytes(c.d_dig.to_host().view(np.uint64).reshape(c.k, 4))
        assert c.digests[0] == keccak.keccak256(c.msgs[0]) and c.digests[-1] == keccak.keccak256(c.msgs[-1])
        c.init, _claims = S.statement(c.msgs, c.digests)
        write_chip(c)
        prove(c)
    for _ in range(args.reps):
        for c in cases.values():
            c.chip_ms.append(write_chip(c))
    for _ in range(args.reps):
        for c in cases.values():
            c.prove.append(prove(c))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name, c in cases.items():
        trace_ms, chip_ms = statistics.median(c.trace_ms), statistics.median(c.chip_ms)
        prove_ms = statistics.median(r[0] for r in c.prove)
        mid = min(c.prove, key=lambda r: abs(r[0] - prove_ms))
        t0 = time.perf_counter()
        rc = S.verify_keccak256(c.msgs, c.digests, mid[1], params=blob)
        verify_ms = (time.perf_counter() - t0) * 1e3
        written = rows * width * 4
        split = kernel_split(args.kernel_stats, name) if args.kernel_stats else {}
        chain, rk = split.get("keccak_sponge_chain_kernel"), split.get("keccak_sponge_rows_kernel")
        longest = dists[name][1]
        line = {"distribution": name, "messages": c.k, "blocks": nb, "sponge_rows": rows, "sponge_columns": width, "chip_rows": chip_rows,
                "reps": args.reps, "sponge_trace_call_ms_median": round(trace_ms, 4), "sponge_trace_call_ms_all": [round(v, 4) for v in c.trace_ms],
                "chain_kernel_us_avg": None if chain is None else round(chain[1] / 1e3, 2),
                "chain_kernel_us_min": None if chain is None else round(chain[2] / 1e3, 2),
                "chain_us_per_dependent_permutation": None if chain is None else round(chain[1] / 1e3 / longest, 3),
                "rows_kernel_us_avg": None if rk is None else round(rk[1] / 1e3, 2), "rows_kernel_us_min": None if rk is None else round(rk[2] / 1e3, 2),
                "rows_kernel_bytes_written": written, "rows_kernel_write_TB_per_s": None if rk is None else round(written / rk[1] / 1e3, 3),
                "profiler_calls": None if rk is None else rk[0], "hbm_nominal_peak_TB_per_s": HBM_PEAK_TBPS,
                "chip_rows_ms_median": round(chip_ms, 4), "chip_rows_write_TB_per_s": round(chip_rows * chip_width * 4 / chip_ms / 1e9, 3),
                "prove_ms_median": round(prove_ms, 3), "prove_ms_all": [round(r[0], 3) for r in c.prove],
                "stages_ms": {a: round(b, 3) for a, b in mid[2].items()}, "init_words": int(c.init.size), "proof_words": int(mid[1].size),
                "verify_keccak256_rc": rc, "verify_keccak256_ms": round(verify_ms, 2), "parent": PARENT}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    hal.close()


if __name__ == "__main__":
    main()
