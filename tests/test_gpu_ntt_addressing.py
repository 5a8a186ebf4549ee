"""Addressing of the fused NTT kernels (raiko_amd/csrc/ntt_fused.hpp): every global access is a workgroup-uniform
64-bit base (column, tile, fs / zk row, per-register step) plus a 32-bit lane offset.  What can go wrong is a base that
drops the column or the per-register step, or one that is truncated to 32 bits.

Small cases: 2^18 points, the smallest size that dispatches the nf_* kernels, with 1, 3 and 17 columns so that the
column index enters the uniform base; every output word against the oracle transform (exact, no tolerance).
  * ntt_forward with blow-up 4 and 2 (rk_batch_expand_into_evaluate_ntt: source and destination are distinct buffers)
  * ntt_reverse_from without the zk shift (rk_batch_interpolate_ntt) and with it (rk_pcs_coset_lde_cols: the interpolation
    with the shift fused into its last pass, then the 4x forward transform to 2^20 points)
  * ntt_reverse_from reading a source buffer distinct from its destination: only a proof from device-resident inputs
    that must stay untouched (on_device = 1) calls it that way, so the case is one 2^18-cycle proof whose seal must
    equal the seal of the same segment proven from host arrays (in-place transforms), inputs unchanged afterwards.

Large case: 2^22 points and 260 columns, 4.06 GiB, so the column base passes 2^32 bytes at column 256.  The columns
are cyclic copies of 4 random base columns, so every group of 4 output columns must equal the oracle's 4 base
outputs; the library has no comparison on the device, so the buffer is read back in 64 MiB slices and every word
compared.  One forward (4x expanding) and one inverse pass."""
import numpy as np
import pytest

import oracle_lib as o

pytestmark = pytest.mark.gpu

K = 18
COUNTS = [1, 3, 17]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("expand_bits", [2, 1], ids=["blowup4", "blowup2"])
def test_forward_expanding(hal, orc, expand_bits, count):
    n_in, n = 1 << (K - expand_bits), 1 << K
    rng = np.random.default_rng(1800 + 10 * expand_bits + count)
    x = o.rand_elems(rng, (count, n_in))
    want = np.zeros((count, n), dtype=np.uint32)
    orc.or_batch_expand_into_evaluate_ntt(want.ctypes.data, x.ctypes.data, n_in, count, expand_bits)
    inp = hal.copy_from_elem(x)
    out = hal.alloc_elem(count * n)
    hal.batch_expand_into_evaluate_ntt(out, inp, count, expand_bits)
    assert np.array_equal(out.to_host().reshape(count, n), want)
    assert np.array_equal(inp.to_host().reshape(count, n_in), x)


@pytest.mark.parametrize("count", COUNTS)
def test_reverse_plain(hal, orc, count):
    n = 1 << K
    rng = np.random.default_rng(1850 + count)
    x = o.rand_elems(rng, (count, n))
    want = x.copy()
    orc.or_batch_interpolate_ntt(want.ctypes.data, n, count)
    buf = hal.copy_from_elem(x)
    hal.batch_interpolate_ntt(buf, count)
    assert np.array_equal(buf.to_host().reshape(count, n), want)


@pytest.mark.parametrize("count", COUNTS)
def test_reverse_with_zk_shift(hal, orc, count):
    """coset LDE of a row-major 2^18 x count trace: interpolation with the zk shift fused (zk table row in the uniform
    base), then the 4x forward transform; the oracle runs the three steps one by one"""
    prm = hal.get_params()
    blow = int(prm.blowup_log2)
    n = 1 << K
    rng = np.random.default_rng(1870 + count)
    rows = o.rand_elems(rng, (n, count))
    cols = rows.T.copy()                      # a copy also at count = 1, where the transpose is contiguous as it is
    orc.or_batch_interpolate_ntt(cols.ctypes.data, n, count)
    orc.or_zk_shift(cols.ctypes.data, n, count)
    want = np.zeros((count, n << blow), dtype=np.uint32)
    orc.or_batch_expand_into_evaluate_ntt(want.ctypes.data, cols.ctypes.data, n, count, blow)
    out = hal.alloc_elem(count * (n << blow))
    hal.pcs_coset_lde_cols(out, hal.copy_from_elem(rows), n, count)
    assert np.array_equal(out.to_host().reshape(count, n << blow), want)


def test_reverse_from_a_distinct_source(hal):
    """on_device = 1: the first pass of every interpolation reads the caller's buffer and writes the prover's own"""
    from raiko_amd.segment import synthetic_segment
    seg = synthetic_segment(K, (4, 4, 24), seed=1818)
    want = hal.prove_segment(seg)
    groups = [hal.copy_from_elem(g) for g in seg.groups]
    check = hal.copy_from_elem(seg.check)
    got = hal.prove_segment(seg, device_inputs=(groups, check), consume_inputs=False)
    assert got.size == want.size and np.array_equal(got, want)
    for buf, g in zip(groups, seg.groups):
        assert np.array_equal(buf.to_host().reshape(g.shape), g)
    assert np.array_equal(check.to_host().reshape(seg.check.shape), seg.check)


def test_column_base_beyond_4_gib(hal, orc):
    kin, k, count, nbase = 20, 22, 260, 4
    n_in, n = 1 << kin, 1 << k
    assert 256 * n * 4 == 1 << 32 and count * n * 4 > 1 << 32
    rng = np.random.default_rng(2222)
    x = o.rand_elems(rng, (nbase, n_in))
    want_f = np.zeros((nbase, n), dtype=np.uint32)
    orc.or_batch_expand_into_evaluate_ntt(want_f.ctypes.data, x.ctypes.data, n_in, nbase, 2)
    want_i = want_f.copy()
    orc.or_batch_interpolate_ntt(want_i.ctypes.data, n, nbase)

    inp = hal.copy_from_elem(np.tile(x, (count // nbase, 1)))      # column c holds base column c % 4
    out = hal.alloc_elem(count * n)
    group = np.empty((nbase, n), dtype=np.uint32)

    def check(want, what):
        """the buffer comes back in slices of 4 columns (64 MiB), every word of it compared"""
        hal.sync()
        for g in range(count // nbase):
            hal._ck(hal._lib.rk_d2h(hal._ctx, group.ctypes.data, out.ptr + g * group.nbytes, group.nbytes))
            assert np.array_equal(group, want), "%s: columns %d..%d differ from the oracle's base columns" % (what, nbase * g, nbase * g + 3)

    hal.batch_expand_into_evaluate_ntt(out, inp, count, 2, in_size=n_in)
    check(want_f, "forward")
    hal.batch_interpolate_ntt(out, count, size=n)
    check(want_i, "inverse")
