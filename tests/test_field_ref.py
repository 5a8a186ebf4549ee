"""tests/field_ref.py (plain-integer reference) against the CPU oracle at small sizes, for both extensions
(W = -11, risc0; W = +11, SP1).  The GPU edge tests (test_gpu_arith_edges.py) compare the kernels with field_ref;
this file is what ties field_ref to the conventions the oracle restates.  A disagreement here means the oracle
is wrong."""
import numpy as np
import pytest

import field_ref as F
import oracle_lib as o

P = F.P
M = F.to_mont


@pytest.fixture(params=[0, 1], ids=["risc0", "sp1"])
def preset(request):
    """the oracle configured for one parameter set; yields (W, generator, coset shift, blow-up, fold)"""
    o.oracle_set_params(request.param)
    if request.param == 0:
        yield F.W_RISC0, F.GEN_RISC0, 3, 2, 4
    else:
        yield F.W_SP1, F.GEN_SP1, 31, 1, 1
    o.oracle_set_params()


def up(a):
    return a.ctypes.data_as(o.u32p)


def canon(a):
    return [int(v) for v in o.from_mont(a)]


def ext_rows(a):
    return [tuple(int(v) for v in r) for r in o.from_mont(np.asarray(a).reshape(-1, 4))]


def rand_ext(rng, n=None):
    return o.rand_elems(rng, (4,) if n is None else (n, 4))


EDGE_EXT = [(0, 0, 0, 0), (1, 0, 0, 0), (P - 1, 0, 0, 0), (P - 1, P - 1, P - 1, P - 1), (0, 0, 0, 1), (5, 0, P - 1, 0)]


def test_montgomery_round_trip():
    x = np.array([0, 1, 2, P - 2, P - 1, 12345], dtype=np.uint64)
    assert np.array_equal(F.from_mont(F.to_mont(x)), x)
    orc = o.oracle()
    for v in (0, 1, P - 1, 987654321):
        assert F.to_mont(v) == orc.or_fp_encode(v)
        assert F.from_mont(orc.or_fp_encode(v)) == v


def test_batch_inverse_and_powers():
    rng = np.random.default_rng(1)
    a = rng.integers(1, P, 1000, dtype=np.uint64)
    a[:3] = (1, P - 1, 2)
    assert all(int(x) * int(y) % P == 1 for x, y in zip(a, F.batch_inv(a)))
    e = rng.integers(0, 1 << 32, 500, dtype=np.uint64)
    assert [int(v) for v in F.vpow(137, e)] == [pow(137, int(x), P) for x in e]


def test_ext_mul_inv_pow_match_oracle(preset):
    W = preset[0]
    orc = o.oracle()
    rng = np.random.default_rng(2)
    vals = EDGE_EXT + [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(20)]
    for a in vals:
        for b in vals[:8]:
            got = np.zeros(4, np.uint32)
            am, bm = F.ext_to_mont(a), F.ext_to_mont(b)
            orc.or_fp4_mul(up(am), up(bm), up(got))
            assert F.ext_from_mont(got) == F.ext_mul(a, b, W)
        if any(a):
            got = np.zeros(4, np.uint32)
            am = F.ext_to_mont(a)
            orc.or_fp4_inv(up(am), up(got))
            ai = F.ext_inv(a, W)
            assert F.ext_from_mont(got) == ai
            assert F.ext_mul(a, ai, W) == (1, 0, 0, 0)
    nz = [a for a in vals if any(a)]
    assert [tuple(int(v) for v in r) for r in F.vext_inv_many(np.array(nz, dtype=np.uint64), W)] == \
        [F.ext_inv(a, W) for a in nz]
    x = vals[7]
    assert F.ext_pow(x, 5, W) == F.ext_mul(F.ext_mul(F.ext_mul(x, x, W), F.ext_mul(x, x, W), W), x, W)
    pw = F.ext_powers(x, 37, W)
    assert [tuple(int(v) for v in r) for r in pw] == [F.ext_pow(x, i, W) for i in range(37)]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 8])
def test_roots_and_ntt_match_oracle(k):
    orc = o.oracle()
    assert F.from_mont(orc.or_rou_fwd(k)) == F.root(k)
    n = 1 << k
    rng = np.random.default_rng(10 + k)
    x = o.rand_elems(rng, (n,))
    a = x.copy()
    orc.or_interpolate_ntt(o.ptr(a), n)
    assert canon(a) == F.ntt_interpolate(canon(x))
    b = x.copy()
    orc.or_evaluate_ntt(o.ptr(b), n, 0)
    assert canon(b) == F.ntt_evaluate(canon(x))
    for e in (1, 2, 4):
        if k + e > 10:
            continue
        out = np.zeros(n << e, np.uint32)
        orc.or_batch_expand_into_evaluate_ntt(o.ptr(out), o.ptr(x), n, 1, e)
        assert canon(out) == F.ntt_evaluate(canon(x), e)
    z = x.copy()
    orc.or_zk_shift(o.ptr(z), n, 1)
    assert canon(z) == F.zk_shift(canon(x))
    assert [int(v) for v in F.zk_shift_vec(canon(x))] == F.zk_shift(canon(x))


@pytest.mark.parametrize("k,e", [(k, e) for k in (1, 2, 4, 7, 10) for e in (0, 1, 3) if k + e <= 10])
def test_closed_forms_match_the_dft(k, e):
    """every closed form the GPU tests use at 2^24, against the O(n^2) DFT"""
    n = 1 << k
    v = P - 1
    for q in sorted({0, 1, n // 2, n - 1}):
        col = [0] * n
        col[q] = v
        assert [int(t) for t in F.evaluate_impulse(k, q, v, e)] == F.ntt_evaluate(col, e)
        if e == 0:
            assert [int(t) for t in F.interpolate_impulse(k, q, v)] == F.ntt_interpolate(col)
    assert [int(t) for t in F.evaluate_constant(k, v, e)] == F.ntt_evaluate([v] * n, e)
    alt = [v * (i & 1) for i in range(n)]
    assert [int(t) for t in F.evaluate_alternating(k, v, e)] == F.ntt_evaluate(alt, e)
    if e == 0:
        assert [int(t) for t in F.interpolate_constant(k, v)] == F.ntt_interpolate([v] * n)
        assert [int(t) for t in F.interpolate_alternating(k, v)] == F.ntt_interpolate(alt)
        for m in sorted({0, 1, n - 1}):
            ev, want = F.interpolate_monomial(k, m, v)
            assert [int(t) for t in want] == F.ntt_interpolate([int(t) for t in ev])


def test_closed_form_of_the_oracle_expand():
    """the closed forms against the oracle itself at a size beyond the DFT (2^12, 4x expansion)"""
    orc = o.oracle()
    k, e, v = 12, 2, P - 1
    n = 1 << k
    for name, col, want in [("impulse", None, F.evaluate_impulse(k, n - 1, v, e)),
                            ("constant", np.full(n, v, np.uint64), F.evaluate_constant(k, v, e)),
                            ("alternating", np.arange(n, dtype=np.uint64) % 2 * v, F.evaluate_alternating(k, v, e))]:
        if col is None:
            col = np.zeros(n, np.uint64)
            col[n - 1] = v
        out = np.zeros(n << e, np.uint32)
        orc.or_batch_expand_into_evaluate_ntt(o.ptr(out), o.ptr(F.to_mont(col)), n, 1, e)
        assert np.array_equal(F.from_mont(out), want), name


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 300])
def test_poly_divide_and_horner_match_oracle(preset, n):
    W = preset[0]
    orc = o.oracle()
    rng = np.random.default_rng(20 + n)
    c = rand_ext(rng, n)
    cc = ext_rows(c)
    for z in [(0, 0, 0, 0), (1, 0, 0, 0), (P - 1, 0, 0, 0), (F.root(6), 0, 0, 0), (12345, 0, 0, 0),
              tuple(int(v) for v in rng.integers(0, P, 4))]:
        zm = F.ext_to_mont(z)
        got, rem = c.copy(), np.zeros(4, np.uint32)
        orc.or_poly_divide(o.ptr(got), n, o.ptr(zm), o.ptr(rem))
        q, r = F.poly_divide(cc, z, W)
        assert ext_rows(got) == q and F.ext_from_mont(rem) == r
        qv, rv = F.vpoly_divide(np.array(cc, dtype=np.uint64), z, W)
        assert [tuple(int(t) for t in row) for row in qv] == q and rv == r
        assert r == F.horner(cc, z, W)
        ev = np.zeros(4, np.uint32)
        orc.or_poly_eval(o.ptr(c), n, o.ptr(zm), o.ptr(ev))
        assert F.ext_from_mont(ev) == r
        # q (x - z) + r == f
        back = F.poly_multiply_linear(q[:-1], z, W) if n > 1 else [(0, 0, 0, 0)]
        back[0] = F.ext_add(back[0], r)
        assert back[:n] == cc


def test_batch_evaluate_any_matches_oracle(preset):
    W = preset[0]
    orc = o.oracle()
    rng = np.random.default_rng(30)
    size = 256
    c = o.rand_elems(rng, (2, size))
    c[1] = P - 1
    xs = np.array([F.ext_to_mont(x) for x in [(0, 0, 0, 0), (1, 0, 0, 0), (F.root(8), 0, 0, 0)]] +
                  [rand_ext(rng)], dtype=np.uint32)
    which = np.array([0, 1, 1, 0], np.uint32)
    want = np.zeros((4, 4), np.uint32)
    orc.or_batch_evaluate_any(o.ptr(c), size, o.ptr(which), o.ptr(xs), 4, o.ptr(want))
    for e in range(4):
        x = F.ext_from_mont(xs[e])
        cf = canon(c[which[e]])
        assert F.ext_from_mont(want[e]) == F.horner([F.ext(v) for v in cf], x, W) == F.vhorner_base(cf, x, W)


def test_prefix_products_mix_and_sum_match_oracle(preset):
    W = preset[0]
    orc = o.oracle()
    rng = np.random.default_rng(40)
    n = 50
    a = rand_ext(rng, n)
    a[20] = 0
    got = a.copy()
    orc.or_prefix_products(o.ptr(got), n)
    assert ext_rows(got) == F.prefix_products(ext_rows(a), W)
    count, combos = 64, np.array([0, 2, 2, 1, 0, 2, 1, 1, 2], np.uint32)
    w = combos.size
    inp = np.full((w, count), P - 1, np.uint32)
    out0 = np.full((3, count, 4), P - 1, np.uint32)
    ms, mx = np.full(4, P - 1, np.uint32), np.full(4, P - 1, np.uint32)
    want = out0.copy()
    orc.or_mix_poly_coeffs(o.ptr(want), o.ptr(ms), o.ptr(mx), o.ptr(inp), o.ptr(combos), w, count)
    ref = F.mix_sum(F.from_mont(out0), F.ext_from_mont(ms), F.ext_from_mont(mx), F.from_mont(inp), combos, W)
    assert np.array_equal(F.from_mont(want), ref)
    e = np.full((5, count, 4), P - 1, np.uint32)
    s = np.zeros((4, count), np.uint32)
    orc.or_eltwise_sum_extelem(o.ptr(s), o.ptr(e), count, 5)
    assert np.array_equal(F.from_mont(s), np.full((4, count), 5 * F.from_mont(P - 1) % P))


@pytest.mark.parametrize("count", [1, 5])
def test_fri_folds_match_oracle(preset, count):
    W, gen, _, _, fold_log2 = preset
    orc = o.oracle()
    rng = np.random.default_rng(50 + count)
    A = 1 << fold_log2
    inp = o.rand_elems(rng, (4, A * count))
    for mix in [(0, 0, 0, 0), (1, 0, 0, 0), (P - 1, 0, 0, 0), tuple(int(v) for v in rng.integers(0, P, 4))]:
        want = np.zeros((4, count), np.uint32)
        orc.or_fri_fold(o.ptr(want), o.ptr(inp), count, o.ptr(F.ext_to_mont(mix)))
        assert np.array_equal(F.from_mont(want), F.fri_fold(F.from_mont(inp), count, mix, fold_log2, W))
    for n_out in (1, 2, 8):
        ev = rand_ext(rng, 2 * n_out)
        for beta in [(0, 0, 0, 0), (1, 0, 0, 0), (P - 1, 0, 0, 0), tuple(int(v) for v in rng.integers(0, P, 4))]:
            want = np.zeros((n_out, 4), np.uint32)
            orc.or_fri_fold_evals(o.ptr(want), o.ptr(ev), n_out, o.ptr(F.ext_to_mont(beta)))
            assert np.array_equal(F.from_mont(want), F.fri_fold_evals(F.from_mont(ev), beta, W, gen))


@pytest.mark.parametrize("k,w", [(1, 1), (3, 3), (4, 9)])
def test_pcs_steps_match_oracle(preset, k, w):
    W, gen, shift, blow, _ = preset
    orc = o.oracle()
    rng = np.random.default_rng(60 + k)
    n = 1 << k
    Hh = n << blow
    ev = o.rand_elems(rng, (n, w))
    lde = np.zeros((Hh, w), np.uint32)
    orc.or_pcs_coset_lde_rows(o.ptr(lde), o.ptr(ev), n, w)
    lc = F.from_mont(lde)
    for c in range(w):
        nat = F.coset_lde_natural([int(v) for v in F.from_mont(ev[:, c])], blow, shift, gen)
        assert [int(lc[r, c]) for r in range(Hh)] == F.to_bitrev_order(nat)
    pts = [tuple(int(v) for v in rng.integers(0, P, 4)), (0, 0, 0, 0), (1234, 0, 0, 0)]
    ys = np.zeros((len(pts), w, 4), np.uint32)
    for j, z in enumerate(pts):
        orc.or_pcs_eval_at(o.ptr(ys[j]), o.ptr(lde), Hh, w, o.ptr(F.ext_to_mont(z)))
        assert ext_rows(ys[j]) == F.pcs_eval_at(lc, Hh, blow, z, shift, gen, W)
    alpha = rand_ext(rng)
    ro0 = rand_ext(rng, Hh)
    want = ro0.copy()
    pm = np.array([F.ext_to_mont(z) for z in pts], np.uint32)
    orc.or_pcs_reduce_openings(o.ptr(want), o.ptr(lde), Hh, w, len(pts), o.ptr(pm), o.ptr(ys), o.ptr(alpha), 7)
    ref = F.pcs_reduce_openings(F.from_mont(ro0), lc, Hh, pts, F.from_mont(ys), F.ext_from_mont(alpha), 7, shift, gen, W)
    assert np.array_equal(F.from_mont(want), ref)
