"""The Poseidon2 kernels of all four instances at the worst-case values of their unreduced arithmetic, on the device:
the aimed cases of tests/p2_edges.py (round-3 external constants solved so that a chosen input enters the partial
rounds at chosen raw cells; diagonals and internal constants whose derived words sit at the edge of the centred
range) through every kernel that runs p2::Core::permute on inputs a test can choose.  Every output word is checked
against the oracle under the same blob and against the plain-integer reference E.permute.

The device build differs from the host build exactly in the arithmetic these cases stress: smadk / smulk / madk are
inline-asm v_mad_i64_i32 / v_mad_u64_u32, fold64 has an asm barrier, and KStream reads the derived words from scalar
registers.  No table family here is refused by the parameter blob (it only checks that entries are below p)."""
import numpy as np
import pytest

import oracle_lib as o
import p2_chip_ref as R
import p2_edges as E
from raiko_amd import p3
from raiko_amd.hal import HipHal

pytestmark = pytest.mark.gpu

P = E.P
PATTERNS = ["alt_h", "mixed", "small", "sign_upd"]
LANES = [0, 63, 64, 255, 256]
ROWS = 300


@pytest.fixture()
def cfg():
    """a context of its own and the oracle under one blob; both back to risc0's defaults afterwards"""
    h = HipHal(0)

    def apply(w, m4, tabs):
        m = E.mont_tables(*tabs)
        kw = dict(p2_width=w, p2_m4=m4, p2_rc_ext=m[0], p2_rc_int=m[1], p2_diag=m[2])
        preset = 0 if w == 24 else 1
        o.oracle_set_params(preset, **kw)
        return h.set_params(preset, **kw)

    yield h, apply
    h.close()
    o.oracle_set_params()


def gpu_input(w):
    """the aimed input: a rate's worth of chosen cells, the capacity zero (what hash_rows and, at width 24, hash_fold
    put in the state); at width 16 the same state is the compression of the children (x[:8], 0)"""
    _, base = E.base_tables(w)
    rate = w - 8
    return base[:rate] + [0] * (w - rate)


def cases(emu, w, m4):
    fams = E.table_families(w, m4)
    out = []
    for label, tabs, inp, raw in E.aimed_cases(emu, w, m4, families={f: fams[f] for f in ("preset", "worst")}, inp=gpu_input(w)):
        if label.split("/")[1] in PATTERNS:
            out.append((label, tabs, inp))
    return out


def mont(x):
    return o.to_mont(np.array([int(v) for v in x], dtype=np.uint64))


def digest_ref(inp, m4, tabs):
    return [int(x) for x in mont(E.permute(inp, m4, *tabs)[:8])]


def check_hash_rows(h, orc, rng, w, m4, tabs, inp, cols, label):
    rate = w - 8
    m = o.rand_elems(rng, (cols, ROWS))
    for lane in LANES:
        m[:rate, lane] = mont(inp[:rate])
    want = np.zeros((ROWS, 8), dtype=np.uint32)
    orc.or_hash_rows(o.ptr(want), o.ptr(m), ROWS, cols)
    out = h.alloc_elem(ROWS * 8)
    h.hash_rows(out, h.copy_from_elem(m), ROWS, cols)
    got = out.to_host().reshape(ROWS, 8)
    assert np.array_equal(got, want), (label, cols)
    if cols == rate:
        ref = digest_ref(inp, m4, tabs)
        for lane in LANES:
            assert [int(x) for x in got[lane]] == ref, (label, lane)


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_hash_rows_fold_and_mmcs_at_aimed_entries(cfg, orc, emu, w, m4):
    """hash_rows_kernel (the aimed row at lanes 0, 63, 64, 255, 256 of 300; cols = rate, and 2 x rate with the aim on
    the first permutation), hash_fold_kernel through rk_hash_fold (the aimed parent's children written by the test),
    hash_rows_multi_kernel through rk_mmcs_commit (the aim on a leaf row of a two-matrix commitment)"""
    h, apply = cfg
    rate = w - 8
    for i, (label, tabs, inp) in enumerate(cases(emu, w, m4)):
        apply(w, m4, tabs)
        rng = np.random.default_rng(100 * i + w + m4)
        ref = digest_ref(inp, m4, tabs)
        check_hash_rows(h, orc, rng, w, m4, tabs, inp, rate, label)
        check_hash_rows(h, orc, rng, w, m4, tabs, inp, 2 * rate, label)
        # rk_hash_fold: 64 parents from 128 children; parent 37 (heap index 64 + 37) has the aimed children
        size = 128
        nodes = o.rand_elems(rng, (2 * size, 8))
        parent = 64 + 37
        nodes[2 * parent] = mont(inp[:8])
        nodes[2 * parent + 1] = mont(inp[8:16])
        want = nodes.copy()
        orc.or_hash_fold(o.ptr(want), size, size // 2)
        dn = h.copy_from_elem(nodes)
        h.hash_fold(dn, size, size // 2)
        got = dn.to_host().reshape(2 * size, 8)
        assert np.array_equal(got[size // 2: size], want[size // 2: size]), label
        assert [int(x) for x in got[parent]] == ref, label
        # rk_mmcs_commit: two row-major matrices of 256 rows whose rows at 200 concatenate to the aimed rate cells
        a, b = o.rand_elems(rng, (256, 5)), o.rand_elems(rng, (256, rate - 5))
        a[200], b[200] = mont(inp[:5]), mont(inp[5:rate])
        from test_mmcs import oracle_commit
        want = oracle_commit([(a, True), (b, True)])
        nodes_d, root = h.mmcs_commit([(h.copy_from_elem(a), 256, 5, 1), (h.copy_from_elem(b), 256, rate - 5, 1)])
        got = nodes_d.to_host().reshape(512, 8)
        assert np.array_equal(got[1:], want[1:]) and np.array_equal(root, want[1]), label
        assert [int(x) for x in got[256 + 200]] == ref, label


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_chip_trace_at_aimed_entries(cfg, emu, w, m4):
    """p2_chip_trace_kernel on the aimed input states (any n x W), a row of p - 1 and random rows: every column against
    p2_chip_ref.chip_trace, under the preset and the worst tables"""
    h, apply = cfg
    for label, tabs, inp in cases(emu, w, m4):
        if not label.endswith("/alt_h") and not label.endswith("/sign_upd"):
            continue
        apply(w, m4, tabs)
        rng = np.random.default_rng(w + m4)
        x = rng.integers(0, P, size=(70, w)).astype(np.uint64)
        x[0] = inp
        x[1] = P - 1
        x[64] = inp
        d_rows, width = p3.poseidon2_chip_trace(h, o.to_mont(x))
        got = o.from_mont(d_rows.to_host().reshape(x.shape[0], width))
        want = R.chip_trace(x, R.tables_of())
        assert np.array_equal(got, want.astype(np.uint32)), label
        out_col = width - 1 - w
        assert [int(v) for v in got[0, out_col: out_col + w]] == E.permute(inp, m4, *tabs), label


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_merkle_heights_under_the_worst_tables(cfg, orc, w, m4):
    """hash_fold_cells_kernel (CellPerm: the levels of up to 4096 parents) and the lane-per-parent levels, under the
    worst table set of the width, heights 1 .. 13.  Its inputs are digests made under the same tables, so no entry
    can be aimed here: this covers the cell-parallel permutation with the edge-valued derived words only."""
    h, apply = cfg
    ext, _ = E.base_tables(w)
    apply(w, m4, (ext, E.WORST[w]["rc_int"], E.WORST[w]["diag"]))
    for log_rows in range(1, 14):
        rows, cols = 1 << log_rows, 3
        rng = np.random.default_rng(9000 + log_rows)
        m = o.rand_elems(rng, (cols, rows))
        want = np.zeros((2 * rows, 8), dtype=np.uint32)
        orc.or_hash_rows(o.ptr(want[rows:]), o.ptr(m), rows, cols)
        size = rows
        while size > 1:
            orc.or_hash_fold(o.ptr(want), size, size // 2)
            size //= 2
        nodes = h.alloc_elem(2 * rows * 8)
        h.merkle_build(nodes, h.copy_from_elem(m), rows, cols)
        assert np.array_equal(nodes.to_host().reshape(2 * rows, 8)[1:], want[1:]), log_rows
