#!/usr/bin/env python3
"""The Keccak-256 padding table at the size of a block's hashing: 2^12 blocks under SP1's full parameter set, as 4096
one-block messages and as one message of 4096 blocks.  What the table costs is measured against what it is put under:
[pad, sponge, chip] and [sponge, chip] are proven over the same bytes in one process, the repetitions ALTERNATING between
the two routes and the two distributions; medians.

Per distribution: rk_keccak_pad_trace (both kernels; a host clock around the call and a device synchronise),
rk_keccak_pad_digests, the host route the device padding replaces (keccak_sponge.pad_blocks and the upload of its blocks),
rk_p3_prove of both table sets over device rows, verify_keccak256_words.  The split of the trace call into its two
kernels comes from a profiler run of its own:
  rocprofv3 --kernel-trace --stats -f csv -d DIR/<dist> -o kp -- python tools/bench_keccak_pad.py --kernels-only --dist <dist>
for <dist> in 4096x1 1x4096, then --kernel-stats DIR on the timed run (without it the split is null: not measured).
Appends one JSON line per distribution to profiles/keccak_pad_bench.jsonl.
  python tools/bench_keccak_pad.py [--log-blocks 12] [--reps 5] [--kernel-stats DIR] [--out profiles/keccak_pad_bench.jsonl]"""
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

from raiko_amd import hal as H, keccak, keccak_chip as K, keccak_pad as KP, keccak_sponge as S, p3  # noqa: E402

KERNELS = ("keccak_pad_blocks_kernel", "keccak_pad_rows_kernel")


def messages(n_msgs, blocks_each, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=136 * (blocks_each - 1) + 50, dtype=np.uint8).tobytes() for _ in range(n_msgs)]


def kernel_split(stats_dir, dist):
    """{kernel: (calls, average ns, min ns)} of the two pad kernels from rocprofv3's kernel stats of one distribution"""
    out = {}
    for path in glob.glob(os.path.join(stats_dir, dist, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for k in KERNELS:
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keccak_pad_bench.jsonl"))
    args = ap.parse_args()
    from raiko_amd.hal import _ptr
    hal = H.HipHal(0)
    blob = hal.set_params(1)
    lib = H._lib.load()
    nb = 1 << args.log_blocks
    dists = {"%dx1" % nb: (nb, 1), "1x%d" % nb: (1, nb)}
    if args.dist is not None:
        dists = {args.dist: dists[args.dist]}
    pad_rows, sponge_rows, chip_rows = KP.min_rows(nb), S.min_rows(nb), K.min_rows(nb)
    logs = [r.bit_length() - 1 for r in (pad_rows, sponge_rows, chip_rows)]
    airs = [KP.keccak_pad_air(blob), S.keccak_sponge_air(blob), K.keccak_chip_air(blob)]
    tables3 = [p3.Table.pinned(a, lg) for a, lg in zip(airs, logs)]
    tables2 = tables3[1:]

    class Case:
        pass

    cases = {}
    for i, (name, (k, each)) in enumerate(dists.items()):
        c = Case()
        c.msgs, c.k = messages(k, each, 100 + i), k
        words, word_first, lens, first = KP.words_of(c.msgs)
        assert int(first[-1]) == nb
        c.n_words = words.size
        c.d_words, c.d_wf, c.d_lens, c.d_first = (hal.copy_from_elem(a) for a in (words, word_first, lens, first))
        c.d_pad, c.d_blocks = hal.alloc_elem(pad_rows * KP.Layout.WIDTH), hal.alloc_elem(nb * 34)
        c.d_host_blocks = None
        c.d_sponge, c.d_states, c.d_outs, c.d_dig = (hal.alloc_elem(n) for n in (sponge_rows * S.Layout.WIDTH, nb * 50, nb * 50, k * 8))
        c.trace_ms, c.dig_ms, c.host_pad_ms, c.upload_ms, c.prove3, c.prove2 = [], [], [], [], [], []
        cases[name] = c

    def pad_trace(c):
        t0 = time.perf_counter()
        H._lib.check(hal._ctx, lib.rk_keccak_pad_trace(hal._ctx, _ptr(c.d_words), c.n_words, _ptr(c.d_wf), _ptr(c.d_lens), _ptr(c.d_first), None,
                                                       c.k, nb, pad_rows, _ptr(c.d_pad), _ptr(c.d_blocks)))
        hal.sync()
        return (time.perf_counter() - t0) * 1e3

    for c in cases.values():
        pad_trace(c)
    for _ in range(args.reps):
        for c in cases.values():
            c.trace_ms.append(pad_trace(c))
    if args.kernels_only:
        print(json.dumps({n: round(statistics.median(c.trace_ms), 4) for n, c in cases.items()}))
        hal.close()
        return

    d_chip = hal.alloc_elem(chip_rows * K.Layout.WIDTH)

    def sponge_and_chip(c, d_blocks):
        H._lib.check(hal._ctx, lib.rk_keccak_sponge_trace(hal._ctx, _ptr(d_blocks), _ptr(c.d_first), None, c.k, nb, sponge_rows, _ptr(c.d_sponge),
                                                          _ptr(c.d_states), _ptr(c.d_outs), _ptr(c.d_dig)))
        H._lib.check(hal._ctx, lib.rk_keccak_chip_trace(hal._ctx, _ptr(c.d_states), None, None, nb, chip_rows, _ptr(d_chip), None))

    def put_digests(c):
        t0 = time.perf_counter()
        H._lib.check(hal._ctx, lib.rk_keccak_pad_digests(hal._ctx, _ptr(c.d_dig), _ptr(c.d_first), c.k, nb, pad_rows, _ptr(c.d_pad)))
        hal.sync()
        return (time.perf_counter() - t0) * 1e3

    def host_route(c):
        """what the device padding replaces: pad_blocks on the host, then the upload of the padded blocks"""
        t0 = time.perf_counter()
        blocks, _first = S.pad_blocks(c.msgs)
        t1 = time.perf_counter()
        c.d_host_blocks = hal.copy_from_elem(blocks.view(np.uint32).reshape(-1))
        hal.sync()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    def prove(c, with_pad):
        """the rows of one route written again (one chip buffer serves both distributions), then the proof alone timed"""
        if with_pad:
            pad_trace(c)
            sponge_and_chip(c, c.d_blocks)
            put_digests(c)
        else:
            sponge_and_chip(c, c.d_host_blocks)
        hal.sync()
        dev = [(_ptr(c.d_pad), logs[0]), (_ptr(c.d_sponge), logs[1]), (_ptr(d_chip), logs[2])][0 if with_pad else 1:]
        t0 = time.perf_counter()
        pf = p3.prove(hal, tables3 if with_pad else tables2, c.init3 if with_pad else c.init2, device_traces=dev)
        return (time.perf_counter() - t0) * 1e3, pf, p3.last_timing(hal)

    for c in cases.values():                                  # warm-up of every shape and route
        host_route(c)
        sponge_and_chip(c, c.d_blocks)
        put_digests(c)
        c.digests = S.digest_bytes(c.d_dig.to_host().view(np.uint64).reshape(c.k, 4))
        assert c.digests[0] == keccak.keccak256(c.msgs[0]) and c.digests[-1] == keccak.keccak256(c.msgs[-1])
        assert np.array_equal(c.d_blocks.to_host(), c.d_host_blocks.to_host())      # device padding = host padding
        c.init3, _claims = KP.statement_words(c.msgs, c.digests)
        c.init2, _claims = S.statement(c.msgs, c.digests)
        prove(c, True)
        prove(c, False)
    for _ in range(args.reps):
        for c in cases.values():
            c.dig_ms.append(put_digests(c))
            h, u = host_route(c)
            c.host_pad_ms.append(h)
            c.upload_ms.append(u)
    for _ in range(args.reps):
        for c in cases.values():
            c.prove3.append(prove(c, True))
            c.prove2.append(prove(c, False))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    med = statistics.median
    for name, c in cases.items():
        p3_ms, p2_ms = med(r[0] for r in c.prove3), med(r[0] for r in c.prove2)
        mid3 = min(c.prove3, key=lambda r: abs(r[0] - p3_ms))
        mid2 = min(c.prove2, key=lambda r: abs(r[0] - p2_ms))
        t0 = time.perf_counter()
        rc = KP.verify_keccak256_words(c.msgs, c.digests, mid3[1], params=blob)
        verify_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        rc2 = S.verify_keccak256(c.msgs, c.digests, mid2[1], params=blob)
        verify2_ms = (time.perf_counter() - t0) * 1e3
        split = kernel_split(args.kernel_stats, name) if args.kernel_stats else {}
        bk, rk = (split.get(k) for k in KERNELS)
        written = pad_rows * KP.Layout.WIDTH * 4
        line = {"distribution": name, "messages": c.k, "blocks": nb, "pad_rows": pad_rows, "pad_columns": KP.Layout.WIDTH, "sponge_rows": sponge_rows,
                "chip_rows": chip_rows, "reps": args.reps,
                "pad_trace_call_ms_median": round(med(c.trace_ms), 4), "pad_trace_call_ms_all": [round(v, 4) for v in c.trace_ms],
                "blocks_kernel_us_avg": None if bk is None else round(bk[1] / 1e3, 2), "blocks_kernel_us_min": None if bk is None else round(bk[2] / 1e3, 2),
                "rows_kernel_us_avg": None if rk is None else round(rk[1] / 1e3, 2), "rows_kernel_us_min": None if rk is None else round(rk[2] / 1e3, 2),
                "rows_kernel_bytes_written": written, "rows_kernel_write_TB_per_s": None if rk is None else round(written / rk[1] / 1e3, 3),
                "profiler_calls": None if rk is None else rk[0],
                "pad_digests_call_ms_median": round(med(c.dig_ms), 4),
                "host_pad_blocks_ms_median": round(med(c.host_pad_ms), 3), "host_blocks_upload_ms_median": round(med(c.upload_ms), 3),
                "prove_pad_sponge_chip_ms_median": round(p3_ms, 3), "prove_pad_sponge_chip_ms_all": [round(r[0], 3) for r in c.prove3],
                "prove_sponge_chip_ms_median": round(p2_ms, 3), "prove_sponge_chip_ms_all": [round(r[0], 3) for r in c.prove2],
                "pad_share_of_proof": round((p3_ms - p2_ms) / p3_ms, 4),
                "stages_ms_pad_sponge_chip": {a: round(b, 3) for a, b in mid3[2].items()},
                "stages_ms_sponge_chip": {a: round(b, 3) for a, b in mid2[2].items()},
                "init_words_pad_sponge_chip": int(c.init3.size), "init_words_sponge_chip": int(c.init2.size),
                "proof_words_pad_sponge_chip": int(mid3[1].size), "proof_words_sponge_chip": int(mid2[1].size),
                "verify_keccak256_words_rc": rc, "verify_keccak256_words_ms": round(verify_ms, 2),
                "verify_keccak256_rc": rc2, "verify_keccak256_ms": round(verify2_ms, 2)}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    hal.close()


if __name__ == "__main__":
    main()
