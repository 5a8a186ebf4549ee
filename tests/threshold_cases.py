"""TEST INFRASTRUCTURE: the inputs that take the host code in front of the kernels across its launch thresholds -- the
size at which an entry point starts a second launch, a strided loop, or another instance of a kernel.

tests/test_launch_thresholds.py (no GPU) reads the thresholds out of the sources (`constants`) and proves that every
shape and seed below lies on the intended side of them; the GPU tests import the same shapes and seeds:

  code fingerprint   S1, S2, S3_SHAPES, chunk_slot          tests/test_gpu_code_fingerprint.py
  grinds             GRIND_BITS, GRIND_SEEDS, grind_*       tests/test_gpu_grind_batches.py
  rk_scatter         scatter_entries, scatter_case          tests/test_gpu_grind_batches.py
  PCS evaluation     PCS_ROW_MAJOR, PCS_COL_MAJOR           tests/test_gpu_pcs.py
  fri_reduce_kernel  FRI_SHARDS, fri_shard, fri_setup       tests/test_gpu_fri_widths.py"""
import ctypes as C
import os
import re

import numpy as np

import oracle_lib as o
import p2_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raiko_amd", "csrc")


# ---------------------------------------------------------------------------------------------- constants from the sources
def _find(text, pattern, what):
    m = re.search(pattern, text)
    assert m, "not found in the sources: " + what
    return int(m.group(1))


def constants():
    """the thresholds as the sources state them (a renamed or reshaped expression fails here, not silently)"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("code_cache.hip", "kernels_hash.hip", "kernels_poly.hip", "kernels_scan.hip",
                                                           "kernels_pcs.hip", "p3_kernels.hpp")}
    k = {}
    for name in ("FP_CHUNK", "FP_TPB", "FP_MAX_BLOCKS"):
        k[name] = _find(src["code_cache.hip"], r"constexpr unsigned %s = (\d+);" % name, name)
    # const uint64_t batch = (uint64_t)1 << (bits + 2 < 16 ? 16 : bits + 2);   in pow_grind and in duplex_grind
    batches = re.findall(r"batch = \(uint64_t\)1 << \(bits \+ (\d+) < (\d+) \? (\d+) : bits \+ (\d+)\);", src["kernels_hash.hip"])
    assert len(batches) == 2 and batches[0] == batches[1], "the grinds' batch expression"
    a, b, c, d = (int(v) for v in batches[0])
    assert a == d and b == c
    k["GRIND_EXTRA_BITS"], k["GRIND_MIN_LOG_BATCH"] = a, b
    k["POLY_TPB"] = _find(src["kernels_poly.hip"], r"constexpr int TPB = (\d+);", "TPB")
    k["GRID_CAP"] = _find(src["kernels_poly.hip"], r"grid_for\(size_t n, unsigned cap = (\d+)\)", "grid_for's cap")
    # unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 16384);   in scatter, both kernels on dim3(256)
    m = re.search(r"grid = \(unsigned\)std::min<size_t>\(\(n \+ (\d+)\) / (\d+), (\d+)\);", src["kernels_scan.hip"])
    assert m, "scatter's grid expression"
    assert int(m.group(1)) + 1 == int(m.group(2))
    k["SCATTER_TPB"], k["SCATTER_GRID"] = int(m.group(2)), int(m.group(3))
    assert len(re.findall(r"scatter_\w+_kernel, dim3\(grid\), dim3\(%d\)" % k["SCATTER_TPB"], src["kernels_scan.hip"])) == 2
    k["BARY_Y"] = _find(src["kernels_pcs.hip"], r"BARY_Y = (\d+)[;,]", "BARY_Y")
    k["BARYC_THREADS"] = _find(src["kernels_pcs.hip"], r"BARYC_THREADS = (\d+)[;,]", "BARYC_THREADS")
    # rows_per_chunk = cols ? max(BARYC_THREADS, (h + 63) / 64) : max(BARY_Y * 16, (h + 1023) / 1024)
    m = re.search(r"rows_per_chunk = cols \? std::max<size_t>\(BARYC_THREADS, \(h \+ (\d+)\) / (\d+)\) : "
                  r"std::max<size_t>\(BARY_Y \* (\d+), \(h \+ (\d+)\) / (\d+)\);", src["kernels_pcs.hip"])
    assert m, "pcs_eval_at's rows_per_chunk expression"
    k["BARYC_CHUNKS"], k["BARY_MIN_SWEEPS"], k["BARY_CHUNKS"] = int(m.group(2)), int(m.group(3)), int(m.group(5))
    assert int(m.group(1)) + 1 == k["BARYC_CHUNKS"] and int(m.group(4)) + 1 == k["BARY_CHUNKS"]
    k["FRI_REDUCE_TPB"] = _find(src["p3_kernels.hpp"], r"FRI_REDUCE_TPB = (\d+)[;,]", "FRI_REDUCE_TPB")
    return k


def bary_rows_per_chunk(k, h, cols):
    """pcs_eval_at's split of the h rows of the low coset into chunks, one workgroup each"""
    if cols:
        return max(k["BARYC_THREADS"], (h + k["BARYC_CHUNKS"] - 1) // k["BARYC_CHUNKS"])
    return max(k["BARY_Y"] * k["BARY_MIN_SWEEPS"], (h + k["BARY_CHUNKS"] - 1) // k["BARY_CHUNKS"])


# ---------------------------------------------------------------------------------------------- the code fingerprint
# (po2, widths, seed) of synthetic_segment; the code group is groups[1], (columns, 2^po2), its flat C index the word index
S1 = (8, (16, 17, 32), 611)            # 4 352 words: one whole chunk and a partial one of 256 words
S2 = (14, (16, 257, 32), 612)          # 4 210 688 words: 1 028 chunks, workgroups 0..3 take a second one
S3_SHAPES = [S1, (12, (16, 16, 32), 613)]   # proven from an address one word past a 16-byte boundary
CHUNK = 4096                           # == FP_CHUNK (asserted in tests/test_launch_thresholds.py): literal indices below
S2_PASS_INDICES = [0, 4095, 4096, 1023 * 4096 + 7, 1024 * 4096, 1025 * 4096 + 4095, -1]    # -1: the last word
S2_ORACLE_INDICES = [1024 * 4096, -1]  # the variants whose seal is compared with the oracle's
SLOT_LANES = [0, 63, 64, 255]


def code_words(shape):
    po2, widths, _ = shape
    return widths[1] << po2


def chunk_slot(t, q, e, tpb=256):
    """word index within a chunk of lane t's register slot w[4 q + e]"""
    return 4 * (t + tpb * q) + e


def fp_chunks(k, words):
    return (words + k["FP_CHUNK"] - 1) // k["FP_CHUNK"]


def fp_blocks(k, words):
    return min(fp_chunks(k, words), k["FP_MAX_BLOCKS"])


def bumped(code, index, by=1):
    """a copy of the code group with `by` added mod p to the word at flat index `index`"""
    out = code.copy()
    flat = out.reshape(-1)
    flat[index] = (int(flat[index]) + by) % o.P
    return out


def swapped(code, i, j, n=1):
    """a copy with the n words from i exchanged with the n words from j; the two runs differ"""
    out = code.copy()
    flat, src = out.reshape(-1), code.reshape(-1)
    assert not np.array_equal(src[i: i + n], src[j: j + n])
    flat[i: i + n], flat[j: j + n] = src[j: j + n], src[i: i + n]
    return out


# ---------------------------------------------------------------------------------------------- the grinds
GRIND_BITS = 14
# (width, m4) -> grind -> [(seed, the oracle's nonce)]: no hit among the first 2^16 candidates, found by scanning seeds
# upward with the oracle's literal search (about one seed in 55: e^-4); "first": an ordinary seed beside them
GRIND_SEEDS = {
    (16, 1): {"duplex": [(7014, 69594), (7035, 94106)], "pow": [(8039, 69708)]},
    (24, 0): {"duplex": [(7255, 87531)], "pow": [(8251, 93972)]},
    (24, 1): {"duplex": [(7014, 76801)], "pow": [(8034, 76370)]},
    (16, 0): {"duplex": [(7020, 87901)], "pow": [(8001, 76071)]},
}
GRIND_FIRST_SEEDS = {"duplex": 7000, "pow": 8000}


def grind_batch(k, bits):
    return 1 << max(k["GRIND_MIN_LOG_BATCH"], bits + k["GRIND_EXTRA_BITS"])


def grind_params(w, m4):
    """(preset, overrides) of the instance under the library's own tables, as tests/test_gpu_p2_kept_cells.py applies them"""
    m = E.mont_tables(*E.preset_tables(w, m4))
    return (0 if w == 24 else 1), dict(p2_width=w, p2_m4=m4, p2_pad_free=0, p2_rc_ext=m[0], p2_rc_int=m[1], p2_diag=m[2])


def duplex_inputs(w, seed):
    rng = np.random.default_rng(seed)
    state = o.rand_elems(rng, (w,))
    return state, o.rand_elems(rng, (5,))


def pow_cells(w, seed):
    return o.rand_elems(np.random.default_rng(seed), (w,))


def oracle_duplex_grind(w, seed, bits=GRIND_BITS):
    state, inputs = duplex_inputs(w, seed)
    return o.oracle().or_duplex_grind(o.ptr(state), o.ptr(inputs), 5, bits)


def oracle_pow_grind(w, seed, bits=GRIND_BITS):
    cells = pow_cells(w, seed)
    iop = o.OrIop()
    for i in range(w):
        iop.cells[i] = int(cells[i])
    return o.oracle().or_pow_grind(C.byref(iop), bits)


# ---------------------------------------------------------------------------------------------- rk_scatter
SCATTER_EXTRA = 1000                   # entries past one grid: lanes 0..999 of the grid take a second one
SCATTER_INTO = 1 << 20


def scatter_entries(k):
    return k["SCATTER_GRID"] * k["SCATTER_TPB"] + SCATTER_EXTRA


def scatter_case(k, seed=41):
    """(index, offsets, values, start, same_lane, other_group): one entry per cycle; for the k of `same_lane` the entry
    k + grid * tpb -- the second iteration of the lane that wrote k -- targets the word of entry k; for `other_group`
    it targets the word of an entry half a grid away, which a lane of another workgroup wrote"""
    n = scatter_entries(k)
    stride = k["SCATTER_GRID"] * k["SCATTER_TPB"]
    rng = np.random.default_rng(seed)
    offsets = rng.integers(0, SCATTER_INTO, size=n, dtype=np.uint32)
    # every entry past the first grid is such a duplicate, half of each kind (there are only SCATTER_EXTRA of them);
    # 4 M random entries into 1 M words collide everywhere else as well
    same_lane = np.sort(rng.choice(SCATTER_EXTRA, size=SCATTER_EXTRA // 2, replace=False))
    other_group = np.setdiff1d(np.arange(SCATTER_EXTRA), same_lane)
    offsets[same_lane + stride] = offsets[same_lane]
    offsets[other_group + stride] = offsets[other_group + stride // 2]
    values = o.rand_elems(rng, (n,))
    start = o.rand_elems(rng, (SCATTER_INTO,))
    index = np.arange(n + 1, dtype=np.uint32)
    return index, offsets, values, start, same_lane, other_group


# ---------------------------------------------------------------------------------------------- PCS evaluation
PCS_ROW_MAJOR = (17, 3, 2)                       # (k, w, points) added to test_eval_at_and_reduce_openings, both presets
PCS_COL_MAJOR = [(1, 15, 9, 4), (0, 15, 5, 4)]   # (preset, k, w, points) added to test_column_major_forms_equal_the_row_major_ones


# ---------------------------------------------------------------------------------------------- fri_reduce_kernel
# shard -> [(log2 rows, width)] of p3.wide_air(W, seed=W) / p3.wide_trace(air, k, seed=W) tables; SP1's preset
FRI_SHARDS = {"A": [(3, 256), (3, 65), (3, 513)],          # three wide matrices in one round
              "B": [(4, 64), (2, 257), (4, 255)]}          # two heights
FRI_OVER = dict(queries=3, pow_bits=2)
FRI_INIT = [1]
FRI_ROWS_PER_QUERY = {"A": 860, "B": 602}


def fri_shard(name):
    from raiko_amd import p3
    tables = []
    for k, w in FRI_SHARDS[name]:
        air = p3.wide_air(w, seed=w)
        tables.append(p3.Table.from_canonical(air, *p3.wide_trace(air, k, seed=w)))
    return tables, p3.to_mont(np.array(FRI_INIT, dtype=np.uint64))


def fri_setup(name, set_params, prove):
    """(blob, tables, init, proof): `set_params(preset, **over)` -> blob on the side that proves, the oracle set alike"""
    blob = set_params(1, **FRI_OVER)
    o.oracle_set_params(1, **FRI_OVER)
    tables, init = fri_shard(name)
    return blob, tables, init, prove(tables, init)
