"""The census of launch thresholds as code: several entry points switch to a second code path above a size -- a second
launch, a strided loop over chunks, another instance of a kernel.  This file reads the thresholds out of the sources
(threshold_cases.constants) and proves, without a GPU, that the inputs of the GPU tests lie on the intended side of each,
so that a GPU test cannot silently stop crossing a threshold when a constant changes.

  code_cache.hip   code_fingerprint      chunks > FP_MAX_BLOCKS: a workgroup loops over chunks   test_gpu_code_fingerprint.py
  kernels_hash.hip pow / duplex_grind    no hit in the first batch: a second launch, base != 0   test_gpu_grind_batches.py
  kernels_scan.hip scatter               n > grid * 256: grid-stride loop in both kernels        test_gpu_grind_batches.py
  kernels_pcs.hip  pcs_eval_at           rows per chunk above the minimum, <4> instance          test_gpu_pcs.py
  fri_tables.hip   fri_reduce_kernel     width against one wave (64) and one piece (256)         test_gpu_fri_widths.py"""
import numpy as np
import pytest

import oracle_lib as o
import p2_edges as E
import threshold_cases as T
from raiko_amd.segment import synthetic_segment


@pytest.fixture(scope="module")
def k():
    return T.constants()


@pytest.fixture()
def params():
    yield o.oracle_set_params
    o.oracle_set_params()


def test_constants_hang_together(k):
    assert k["FP_CHUNK"] == T.CHUNK == 16 * k["FP_TPB"] and k["FP_TPB"] % 64 == 0
    assert k["FP_MAX_BLOCKS"] >= 2
    assert k["SCATTER_TPB"] == k["POLY_TPB"] and k["SCATTER_GRID"] == k["GRID_CAP"]
    assert k["FRI_REDUCE_TPB"] % 64 == 0 and k["FRI_REDUCE_TPB"] > 64
    assert k["BARYC_THREADS"] % 64 == 0


# ---------------------------------------------------------------------------------------------- the code fingerprint
def test_fingerprint_s1_is_a_whole_chunk_beside_a_partial_one(k):
    words = T.code_words(T.S1)
    assert T.fp_chunks(k, words) == 2 == T.fp_blocks(k, words)
    partial = words - k["FP_CHUNK"]
    assert 0 < partial < k["FP_CHUNK"] and partial == 4 * 64           # lanes 0..63 of the partial chunk hold words, slot q = 0 only
    slots = [T.chunk_slot(t, q, e, k["FP_TPB"]) for q in range(4) for e in range(4) for t in T.SLOT_LANES]
    assert len(set(slots)) == 64 and max(slots) == k["FP_CHUNK"] - 1 and min(slots) == 0
    assert {t // 64 for t in T.SLOT_LANES} >= {0, 1, k["FP_TPB"] // 64 - 1} and {t % 64 for t in T.SLOT_LANES} == {0, 63}
    assert all(T.chunk_slot(t, 0, e, k["FP_TPB"]) < partial for t in (0, 63) for e in range(4))
    assert T.chunk_slot(64, 0, 0, k["FP_TPB"]) == partial              # the first word past the input: read as 0


def test_fingerprint_s2_gives_four_workgroups_a_second_chunk(k):
    words = T.code_words(T.S2)
    chunks, blocks = T.fp_chunks(k, words), T.fp_blocks(k, words)
    assert words % k["FP_CHUNK"] == 0 and chunks == k["FP_MAX_BLOCKS"] + 4 and blocks == k["FP_MAX_BLOCKS"]
    where = [(i % words) // k["FP_CHUNK"] for i in T.S2_PASS_INDICES]
    assert where == [0, 0, 1, blocks - 1, blocks, blocks + 1, chunks - 1]
    assert [c // blocks for c in where] == [0, 0, 0, 0, 1, 1, 1]       # the loop iteration that reads the word
    assert [c % blocks for c in where] == [0, 0, 1, blocks - 1, 0, 1, 3]   # the workgroup
    assert all((i % words) // k["FP_CHUNK"] >= blocks for i in T.S2_ORACLE_INDICES)
    # the swaps of tests/test_gpu_code_fingerprint.py: chunk 3 and chunk 1027 are one workgroup's, chunk 0 and 1024 too
    assert 3 % blocks == (chunks - 1) % blocks and 0 == blocks % blocks and chunks - 1 == blocks + 3


def test_fingerprint_s3_shapes(k):
    assert T.S3_SHAPES[0] == T.S1
    words = T.code_words(T.S3_SHAPES[1])
    assert words % k["FP_CHUNK"] == 0 and 1 < T.fp_chunks(k, words) <= k["FP_MAX_BLOCKS"]    # whole chunks, one per workgroup


def test_fingerprint_inputs_are_canonical_and_the_swapped_words_differ():
    for shape in (T.S1, T.S2, T.S3_SHAPES[1]):
        po2, widths, seed = shape
        code = synthetic_segment(po2, widths, seed=seed).groups[1]
        assert code.shape == (widths[1], 1 << po2) and code.flags.c_contiguous and int(code.max()) < o.P
    flat = synthetic_segment(*T.S2[:2], seed=T.S2[2]).groups[1].reshape(-1)
    assert not np.array_equal(flat[: T.CHUNK], flat[1024 * T.CHUNK: 1025 * T.CHUNK])


# ---------------------------------------------------------------------------------------------- the grinds
def test_grind_batch_at_14_bits(k):
    assert T.grind_batch(k, T.GRIND_BITS) == 1 << 16
    assert set(T.GRIND_SEEDS) == set(E.INSTANCES)


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_grind_seeds_find_nothing_in_the_first_batch(k, params, w, m4):
    """the oracle's literal search 0, 1, 2, ... ends in [batch, 2 batch): the kernels' hit comes from the second launch"""
    batch = T.grind_batch(k, T.GRIND_BITS)
    preset, kw = T.grind_params(w, m4)
    params(preset, **kw)
    for seed, nonce in T.GRIND_SEEDS[(w, m4)]["duplex"]:
        assert T.oracle_duplex_grind(w, seed) == nonce and batch <= nonce < 2 * batch
    for seed, nonce in T.GRIND_SEEDS[(w, m4)]["pow"]:
        assert T.oracle_pow_grind(w, seed) == nonce and batch <= nonce < 2 * batch
    assert T.oracle_duplex_grind(w, T.GRIND_FIRST_SEEDS["duplex"]) < batch
    assert T.oracle_pow_grind(w, T.GRIND_FIRST_SEEDS["pow"]) < batch


# ---------------------------------------------------------------------------------------------- rk_scatter
def test_scatter_case_runs_past_one_grid(k, orc):
    stride = k["SCATTER_GRID"] * k["SCATTER_TPB"]
    n = T.scatter_entries(k)
    assert stride < n < 2 * stride and n - stride == T.SCATTER_EXTRA
    index, offsets, values, start, same_lane, other_group = T.scatter_case(k)
    assert index.size == n + 1 and offsets.size == values.size == n and int(offsets.max()) < T.SCATTER_INTO
    assert same_lane.size + other_group.size == T.SCATTER_EXTRA and not np.intersect1d(same_lane, other_group).size
    late = lambda a: a + stride
    assert np.array_equal(offsets[late(same_lane)], offsets[same_lane])
    assert np.array_equal(offsets[late(other_group)], offsets[other_group + stride // 2])
    # entry e is lane e % stride of the grid: the same lane; and workgroup (e % stride) / tpb: another workgroup
    assert np.array_equal(late(same_lane) % stride, same_lane)
    assert not np.any((late(other_group) % stride) // k["SCATTER_TPB"] == (other_group + stride // 2) // k["SCATTER_TPB"])
    want = start.copy()
    orc.or_scatter(o.ptr(want), o.ptr(index), n, o.ptr(offsets), o.ptr(values))
    last = start.copy()
    last[offsets] = values                          # numpy assigns in order: the last of repeated indices holds
    assert np.array_equal(want, last)
    tail = np.arange(stride, n)
    winners = tail[np.array([not np.any(offsets[e + 1:] == offsets[e]) for e in tail])]
    assert winners.size > T.SCATTER_EXTRA * 9 // 10
    assert np.array_equal(want[offsets[winners]], values[winners])    # what the second iteration wrote is what stays


# ---------------------------------------------------------------------------------------------- PCS evaluation
def test_pcs_shapes_leave_the_minimum_chunk(k):
    lo = k["BARY_Y"] * k["BARY_MIN_SWEEPS"]
    kk, w, npts = T.PCS_ROW_MAJOR
    assert T.bary_rows_per_chunk(k, 1 << 16, False) == lo                  # the largest height that still has the minimum
    assert T.bary_rows_per_chunk(k, 1 << kk, False) == 2 * lo             # 128 rows: each sub-row sweeps twice as often
    assert (1 << kk) // T.bary_rows_per_chunk(k, 1 << kk, False) == k["BARY_CHUNKS"]
    for preset, kk, w, npts in T.PCS_COL_MAJOR:
        assert T.bary_rows_per_chunk(k, 1 << 14, True) == k["BARYC_THREADS"]
        assert T.bary_rows_per_chunk(k, 1 << kk, True) == 2 * k["BARYC_THREADS"]   # two strides of the workgroup's lanes
        assert npts == 4                                                   # bary_dot_cols_kernel<4>
    assert {c[0] for c in T.PCS_COL_MAJOR} == {0, 1}


# ---------------------------------------------------------------------------------------------- fri_reduce_kernel
@pytest.mark.parametrize("name", list(T.FRI_SHARDS))
def test_fri_shards_put_their_widths_around_a_wave_and_a_piece(k, params, name):
    from raiko_amd import fri_open, fri_reduce, fri_transcript, hal, p3
    tpb = k["FRI_REDUCE_TPB"]
    blob, tables, init, pf = T.fri_setup(name, hal.make_params, o.oracle_p3_prove)
    assert p3.verify(tables, pf, init, params=blob) == 0
    st = fri_reduce.statement(tables, pf, init, blob)
    widths = [m.width for m in st.layout if m.batch == 0]
    assert widths == [w for _, w in T.FRI_SHARDS[name]]
    sz = fri_reduce.sizes(st)
    assert sz["rows_per_query"] == T.FRI_ROWS_PER_QUERY[name]
    rounds = [m.rd for m in st.layout if m.batch == 0]
    if name == "A":
        assert sz["n_slots"] == 11 and len(set(rounds)) == 1 and min(widths) > 64    # three wide matrices in one round
    else:
        assert len(set(rounds)) == 2
        wide = [m.rd for m in st.layout if m.width > 64]
        assert len(wide) >= 2                                                    # two or more wide matrices
    for mod in (fri_open, fri_transcript):
        s2 = mod.statement(tables, pf, init, blob)
        assert mod.sizes(s2)["rows_per_query"] == sz["rows_per_query"]
        assert len(mod.witness(s2)) == len(mod.heights(s2))
    both = [w for s in T.FRI_SHARDS.values() for _, w in s]
    assert any(w % 64 == 0 and w < tpb for w in both) and any(w % 64 == 1 and w < tpb for w in both)
    assert {tpb - 1, tpb, tpb + 1} <= set(both) and max(both) > 2 * tpb
