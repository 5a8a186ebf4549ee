"""The kernels that run the kept-cell and zero-aware forms of p2::Core::permute, all four instances, against the oracle
under the same parameter blob: hash_rows_kernel at every column count where a row takes another path (no block, only a
partial block, exactly one block, chained blocks with and without a partial one), both sponge kinds; the lane-per-parent
folds and the cell-parallel top through rk_merkle_build; compress_inject_kernel through a commitment of a tall and a
short matrix; one proof-of-work search of each kind; uni-stark proofs under the width-24 set with two in flight, which
once changed from run to run.  300 rows: the last workgroup is partial, and the compared rows
include lanes 0, 63, 64, 255, 256.  The host side is tests/test_p2_ext_layer.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as o
import p2_edges as E
from raiko_amd import _lib
from raiko_amd.hal import HipHal

pytestmark = pytest.mark.gpu

ROWS = 300
COLS = {24: [0, 1, 15, 16, 17, 32, 48], 16: [0, 1, 7, 8, 9, 16, 24]}


@pytest.fixture()
def cfg():
    """a context of its own and the oracle under one blob; both back to risc0's defaults afterwards"""
    h = HipHal(0)

    def apply(w, m4, pad_free=0):
        m = E.mont_tables(*E.preset_tables(w, m4))
        kw = dict(p2_width=w, p2_m4=m4, p2_pad_free=pad_free, p2_rc_ext=m[0], p2_rc_int=m[1], p2_diag=m[2])
        preset = 0 if w == 24 else 1
        o.oracle_set_params(preset, **kw)
        return h.set_params(preset, **kw)

    yield h, apply
    h.close()
    o.oracle_set_params()


@pytest.mark.parametrize("pad_free", [0, 1])
@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_hash_rows_at_every_block_count(cfg, orc, w, m4, pad_free):
    h, apply = cfg
    apply(w, m4, pad_free)
    rng = np.random.default_rng(31 * w + 2 * m4 + pad_free)
    for cols in COLS[w]:
        m = o.rand_elems(rng, (max(cols, 1), ROWS))[:cols]
        m = np.ascontiguousarray(m).reshape(cols, ROWS)
        if cols:
            m[:, 0] = o.P - 1                      # a row of the largest canonical cells (Montgomery words p - 1)
            m[:, 255] = 0
        want = np.zeros((ROWS, 8), dtype=np.uint32)
        orc.or_hash_rows(o.ptr(want), o.ptr(m if cols else np.zeros(1, dtype=np.uint32)), ROWS, cols)
        out = h.alloc_elem(ROWS * 8)
        src = h.copy_from_elem(m) if cols else h.alloc_elem(1)
        h.hash_rows(out, src, ROWS, cols)
        got = out.to_host().reshape(ROWS, 8)
        assert np.array_equal(got, want), (cols, pad_free)


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_merkle_build_folds_and_top(cfg, orc, w, m4):
    """2^14 rows of 17 columns: leaves with one chained block and a partial one, lane-per-parent folds down to the
    cell-parallel top"""
    h, apply = cfg
    apply(w, m4)
    rows, cols = 1 << 14, 17
    m = o.rand_elems(np.random.default_rng(w + m4), (cols, rows))
    want = np.zeros((2 * rows, 8), dtype=np.uint32)
    orc.or_hash_rows(o.ptr(want[rows:]), o.ptr(m), rows, cols)
    size = rows
    while size > 1:
        orc.or_hash_fold(o.ptr(want), size, size // 2)
        size //= 2
    nodes = h.alloc_elem(2 * rows * 8)
    h.merkle_build(nodes, h.copy_from_elem(m), rows, cols)
    assert np.array_equal(nodes.to_host().reshape(2 * rows, 8)[1:], want[1:])


@pytest.mark.parametrize("pad_free", [0, 1])
@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_mmcs_commit_tall_and_short(cfg, w, m4, pad_free):
    """a 512-row matrix of two blocks and a partial one and a 64-row matrix of exactly one block: hash_rows_multi_kernel
    on both shapes, the folds, and compress_inject_kernel where the short matrix joins"""
    from test_mmcs import oracle_commit
    h, apply = cfg
    apply(w, m4, pad_free)
    rate = w - 8
    rng = np.random.default_rng(5 * w + m4 + pad_free)
    tall, short = o.rand_elems(rng, (512, 2 * rate + 3)), o.rand_elems(rng, (64, rate))
    want = oracle_commit([(tall, True), (short, True)])
    nodes_d, root = h.mmcs_commit([(h.copy_from_elem(tall), 512, 2 * rate + 3, 1), (h.copy_from_elem(short), 64, rate, 1)])
    got = nodes_d.to_host().reshape(1024, 8)
    assert np.array_equal(got[1:], want[1:]) and np.array_equal(root, want[1])


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_grinds(cfg, orc, w, m4):
    """rk_pow_grind and rk_duplex_grind (12 bits) against the oracle's literal searches"""
    h, apply = cfg
    apply(w, m4)
    rng = np.random.default_rng(77 + w + m4)
    bits = 12
    iop = o.OrIop()
    cells = o.rand_elems(rng, (w,))
    for i in range(w):
        iop.cells[i] = int(cells[i])
    want = orc.or_pow_grind(C.byref(iop), bits)
    nonce = C.c_uint32(0)
    _lib.check(h._ctx, h._lib.rk_pow_grind(h._ctx, cells.ctypes.data_as(_lib.u32p), bits, C.byref(nonce)))
    assert nonce.value == want
    state, inputs = o.rand_elems(rng, (w,)), o.rand_elems(rng, (5,))
    assert h.duplex_grind(state, inputs, bits) == orc.or_duplex_grind(o.ptr(state), o.ptr(inputs), 5, bits)


def test_two_proofs_in_flight_repeat_under_the_width_24_set():
    """three rv32i-cf shards under risc0's set (width 24, zero-padding sponge) through p3.prove_shards: with two and
    three proofs in flight, call after call, the words are those of one proof at a time.  While p2 KStream issued its
    scalar loads from inline asm, hash_rows_multi_kernel copied a chunk's registers before the load had landed whenever a
    second proof contended for memory: the second call with batch = 2 gave other words from the permutation root on, or
    a proof that did not verify.  Whether a stale copy shows depends on timing, so this test can pass over the hazard;
    tests/test_p2_kstream.py holds the source"""
    import rv32_cf_programs as CP
    from raiko_amd import p3
    from raiko_amd import executor as X
    from raiko_amd.hal import make_params
    blob = make_params(0, queries=8, pow_bits=6)
    ex = X.execute(CP.cf_program(100), [11, 22, 33, 44], segment_limit_po2=13, record_trace=True)
    shards = X.p3_rv32cf_shards(ex, ext_w=int(blob.ext_w))
    assert len(shards) == 3
    want = p3.prove_shards(shards, blob, batch=1, verify=True)
    for batch in (2, 2, 3, 2):
        got = p3.prove_shards(shards, blob, batch=batch, verify=True)
        for k, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (batch, k)
