"""The NTT, extension-field and PCS kernels at edge values and on every NTT dispatch path, against the exact
reference of tests/field_ref.py (closed forms where they exist), word for word.

Values: "saturated" data are raw Montgomery words p - 1, the largest word a buffer can hold, so every add / sub
runs at the top of its range; challenges and divisor points are field elements (0, 1, -1, roots of unity).
NTT entry points are also run on buffers offset by one word (a 4-byte aligned pointer into a larger allocation):
they dispatch on 16-byte alignment, and the offset form takes the general passes (including the scalar form of
the unrolled pass kernel) at sizes where aligned buffers take the fused kernels.  Extension buffers are always
16-byte aligned: those kernels use 16-byte loads."""
import numpy as np
import pytest

import field_ref as F
import oracle_lib as o
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

P = F.P
SAT = P - 1                    # raw word
VSAT = int(F.from_mont(SAT))   # its value


def val(words):
    """values of Montgomery words, which must be canonical: a word p or above is a wrong word even when it is
    congruent to the right one, so this keeps every comparison word for word"""
    words = np.asarray(words)
    assert (words < P).all(), "non-canonical word %d" % int(words.max())
    return F.from_mont(words)


def ext_val(words):
    return tuple(int(v) for v in val(np.asarray(words, dtype=np.uint64)))


def mont(a):
    return F.to_mont(np.asarray(a, dtype=np.uint64))


def upload(hal, words, offset):
    """device buffer holding `words` at word offset 0 or 1; returns (keepalive buffer, address)"""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    buf = hal.alloc_elem(words.size + 4)
    host = np.zeros(words.size + 4, np.uint32)
    host[offset:offset + words.size] = words
    buf.copy_from(host)
    return buf, buf.ptr + 4 * offset


def download(buf, offset, n):
    return buf.to_host()[offset:offset + n]


def ntt_inputs(k, full):
    """structured columns (canonical values) for a transform of 2^k points: (name, column, impulse position)"""
    n = 1 << k
    cols = []
    for q in (sorted({0, 1, n // 2, n - 1}) if full else [n - 1]):
        c = np.zeros(n, np.uint64)
        c[q] = VSAT
        cols.append(("impulse%d" % q, c, q))
    cols.append(("zero", np.zeros(n, np.uint64), None))
    cols.append(("saturated", np.full(n, VSAT, np.uint64), None))
    if k >= 1:
        cols.append(("alternating", np.arange(n, dtype=np.uint64) % 2 * VSAT, None))
    return cols


def pick(k, k_out=None):
    """the columns run at one size: every structured column up to 2^22 output points; at 2^23 and 2^24 (one column
    is 64 MiB there) the impulse at n - 1, the saturated and the alternating column"""
    k_out = k if k_out is None else k_out
    full = ntt_inputs(k, True)
    if k_out <= 22:
        return full
    return [c for c in full if c[0] in ("impulse%d" % ((1 << k) - 1), "saturated", "alternating")]


def want_evaluate(k, name, q, e):
    if name.startswith("impulse"):
        return F.evaluate_impulse(k, q, VSAT, e)
    if name == "zero":
        return np.zeros(1 << (k + e), np.uint64)
    if name == "saturated":
        return F.evaluate_constant(k, VSAT, e)
    return F.evaluate_alternating(k, VSAT, e)


def want_interpolate(k, name, q):
    if name.startswith("impulse"):
        return F.interpolate_impulse(k, q, VSAT)
    if name == "zero":
        return np.zeros(1 << k, np.uint64)
    if name == "saturated":
        return F.interpolate_constant(k, VSAT)
    return F.interpolate_alternating(k, VSAT)


KS = list(range(1, 25))


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("k", KS)
def test_interpolate_structured(hal, k, offset):
    cols = pick(k)
    n = 1 << k
    x = np.stack([mont(c) for _, c, _ in cols])
    if k <= 22:   # monomial evaluations w^(i m): the interpolation is one coefficient
        for m in (1, n - 1):
            ev, _ = F.interpolate_monomial(k, m, VSAT)
            x = np.concatenate([x, mont(ev)[None]])
    buf, addr = upload(hal, x, offset)
    hal.batch_interpolate_ntt(addr, x.shape[0], size=n)
    got = val(download(buf, offset, x.size)).reshape(x.shape[0], n)
    for i, (name, _, q) in enumerate(cols):
        assert np.array_equal(got[i], want_interpolate(k, name, q)), name
    if k <= 22:
        for j, m in enumerate((1, n - 1)):
            assert np.array_equal(got[len(cols) + j], F.interpolate_monomial(k, m, VSAT)[1]), m


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("k", KS)
def test_evaluate_in_place_structured(hal, k, offset):
    cols = pick(k)
    n = 1 << k
    x = np.stack([mont(c) for _, c, _ in cols])
    buf, addr = upload(hal, x, offset)
    hal.batch_evaluate_ntt(addr, len(cols), 0, size=n)
    got = val(download(buf, offset, x.size)).reshape(len(cols), n)
    for i, (name, _, q) in enumerate(cols):
        assert np.array_equal(got[i], want_evaluate(k, name, q, 0)), name


EXPAND = [(k, e) for e in range(5) for k in range(1, 25 - e)
          if e == 2 or k in (1, 2, 5, 9, 10, 13, 14, 16, 17, 18, 19, 20, 21, 22, 24 - e)]


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset1"])
@pytest.mark.parametrize("k,e", EXPAND)
def test_expand_into_evaluate_structured(hal, k, e, offset):
    cols = pick(k, k + e)
    n, N = 1 << k, 1 << (k + e)
    x = np.stack([mont(c) for _, c, _ in cols])
    ib, ia = upload(hal, x, offset)
    ob, oa = upload(hal, np.zeros(len(cols) * N, np.uint32), offset)
    hal.batch_expand_into_evaluate_ntt(oa, ia, len(cols), e, in_size=n)
    got = val(download(ob, offset, len(cols) * N)).reshape(len(cols), N)
    for i, (name, _, q) in enumerate(cols):
        assert np.array_equal(got[i], want_evaluate(k, name, q, e)), (name, k, e)


@pytest.mark.parametrize("k", KS)
def test_round_trip_and_alignment_agree(hal, k):
    """random columns: evaluate(interpolate(x)) == x on both alignments, and at 2^18 .. 2^22 (fused kernels aligned,
    general passes offset) the two alignments give the same words after each step"""
    n = 1 << k
    count = 2 if k <= 20 else 1
    rng = np.random.default_rng(900 + k)
    x = o.rand_elems(rng, (count, n))
    res = []
    for offset in (0, 1):
        buf, addr = upload(hal, x, offset)
        hal.batch_interpolate_ntt(addr, count, size=n)
        mid = download(buf, offset, x.size)
        hal.batch_evaluate_ntt(addr, count, 0, size=n)
        assert np.array_equal(download(buf, offset, x.size), x.reshape(-1)), offset
        res.append(mid)
        del buf
    assert np.array_equal(res[0], res[1])
    if 18 <= k <= 22:
        outs = []
        for offset in (0, 1):
            ib, ia = upload(hal, res[0], offset)
            ob, oa = upload(hal, np.zeros(count * 4 * n, np.uint32), offset)
            hal.batch_expand_into_evaluate_ntt(oa, ia, count, 2, in_size=n)
            outs.append(download(ob, offset, count * 4 * n))
            del ib, ob
        assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("k", [1, 4, 10, 14, 18, 20])
def test_zk_shift_structured(hal, k):
    cols = pick(k)
    n = 1 << k
    x = np.stack([mont(c) for _, c, _ in cols])
    buf = hal.copy_from_elem(x)
    hal.zk_shift(buf, len(cols), size=n)
    got = val(buf.to_host()).reshape(len(cols), n)
    for i, (name, c, _) in enumerate(cols):
        assert np.array_equal(got[i], F.zk_shift_vec(c)), name


def coset_lde_closed_form(kind, k, blow, shift, q=None, m=None):
    """values at the LDE rows (x_r = shift * w_H^bitrev(r)) of the polynomial interpolating a structured column"""
    h, kb = 1 << k, k + blow
    x = F.vmul(F.vpow(F.root(kb), F.bitrev_perm(kb)), shift)
    if kind == "saturated":
        return np.full(h << blow, VSAT, np.uint64)
    if kind == "alternating":       # v/2 (1 - x^(h/2))
        return F.vmul(F.vsub(1, _xpow(x, h // 2)), VSAT * F.inv(2) % P)
    if kind == "monomial":
        return F.vmul(_xpow(x, m), VSAT)
    # impulse at evaluation index q: v L_q(x) = v w^q (x^h - 1) / (h (x - w^q))
    wq = pow(F.root(k), q, P)
    num = F.vmul(F.vsub(_xpow(x, h), 1), VSAT * wq % P * F.inv(h) % P)
    return F.vmul(num, F.batch_inv(F.vsub(x, wq)))


def _xpow(x, e):
    r = np.ones_like(x)
    b = x.copy()
    while e:
        if e & 1:
            r = F.vmul(r, b)
        b = F.vmul(b, b)
        e >>= 1
    return r


@pytest.mark.parametrize("k", [2, 6, 12, 16, 18])
def test_coset_lde_fused_zk_shift_structured(hal, k):
    """pcs_coset_lde_rows / _cols (interpolate with the zk shift fused into its last pass, then expand) on
    structured columns: the LDE of an impulse is a scaled Lagrange basis polynomial, of a constant the constant"""
    p = hal.get_params()
    blow, shift = int(p.blowup_log2), int(p.coset_shift)
    h = 1 << k
    Hh = h << blow
    spec = [("saturated", None, None), ("alternating", None, None), ("impulse", 0, None), ("impulse", h - 1, None),
            ("impulse", h // 2, None), ("monomial", None, 1), ("monomial", None, h - 1), ("impulse", 1, None)]
    cols = []
    for kind, q, m in spec:
        if kind == "saturated":
            c = np.full(h, VSAT, np.uint64)
        elif kind == "alternating":
            c = np.arange(h, dtype=np.uint64) % 2 * VSAT
        elif kind == "monomial":
            c = F.interpolate_monomial(k, m, VSAT)[0]
        else:
            c = np.zeros(h, np.uint64)
            c[q] = VSAT
        cols.append(c)
    w = len(cols)
    want = np.stack([coset_lde_closed_form(kind, k, blow, shift, q, m) for kind, q, m in spec], axis=1)  # (Hh, w)
    ev = mont(np.stack(cols, axis=1))                                                                    # (h, w)
    out = hal.alloc_elem(Hh * w)
    hal.pcs_coset_lde_rows(out, hal.copy_from_elem(ev), h, w)
    assert np.array_equal(val(out.to_host()).reshape(Hh, w), want)
    outc = hal.alloc_elem(Hh * w)
    hal.pcs_coset_lde_cols(outc, hal.copy_from_elem(ev), h, w)
    natural = want[np.argsort(F.bitrev_perm(k + blow))]      # layout 2: columns of natural-order evaluations
    assert np.array_equal(val(outc.to_host()).reshape(w, Hh), natural.T)


# ---------------------------------------------------------------- extension kernels
@pytest.fixture(scope="module", params=[0, 1], ids=["risc0", "sp1"])
def ectx(request):
    """a context of its own under one parameter set: (hal, W, generator, fold log2)"""
    h = H.HipHal(0)
    h.set_params(preset=request.param)
    if request.param == 0:
        yield h, F.W_RISC0, F.GEN_RISC0, 4
    else:
        yield h, F.W_SP1, F.GEN_SP1, 1
    h.close()


def z_points(W, rng):
    return {"zero": (0, 0, 0, 0), "one": (1, 0, 0, 0), "minus_one": (P - 1, 0, 0, 0),
            "root64": (F.root(6), 0, 0, 0), "base": (int(rng.integers(2, P)), 0, 0, 0),
            "ext": tuple(int(v) for v in rng.integers(0, P, 4))}


@pytest.mark.parametrize("count", [1, 63, 64, 65, 64 * 1024 - 1, 64 * 1024 + 1, (1 << 17) + 3])
def test_poly_divide_edges(ectx, count):
    h, W, _, _ = ectx
    rng = np.random.default_rng(count)
    coeffs = np.full((count, 4), SAT, np.uint32)            # saturated words
    cv = val(coeffs)
    for zname, z in z_points(W, rng).items():
        if zname == "ext" and count > 70000 and W == F.W_SP1:
            continue   # the extension-point case runs the Python Horner loop: once per count is enough
        buf = h.copy_from_elem(coeffs)
        rem = h.poly_divide(buf, count, F.ext_to_mont(z))
        q, r = F.vpoly_divide(cv, z, W)
        assert ext_val(rem) == r, zname
        assert np.array_equal(val(buf.to_host()).reshape(count, 4), np.asarray(q, np.uint64)), zname
    # a polynomial with a root at z: g (x - z), remainder 0, quotient g
    for zname in ("one", "root64", "ext"):
        z = z_points(W, rng)[zname]
        g = val(o.rand_elems(rng, (count - 1, 4))) if count > 1 else np.zeros((0, 4), np.uint64)
        f = np.zeros((count, 4), np.uint64)
        f[1:] = g
        f[:-1] = F.vsub(f[:-1], F.vext_mul(g, np.array(z, np.uint64), W))
        buf = h.copy_from_elem(mont(f))
        rem = h.poly_divide(buf, count, F.ext_to_mont(z))
        assert ext_val(rem) == (0, 0, 0, 0), zname
        got = val(buf.to_host()).reshape(count, 4)
        assert np.array_equal(got[:-1], g) and not got[-1].any(), zname


@pytest.mark.parametrize("size", [1, 2, 1 << 15, 1 << 16, 1 << 17])
def test_batch_evaluate_any_edges(ectx, size):
    """sizes around DOT_BLOCKS * TPB * 4 = 2^16, the span of one unrolled step of eval_dot_kernel: below it
    (1, 2, 2^15) only the tail loop runs, at and above it the unrolled loop.  The entry point takes powers of two
    only; a size of 2^16 + 1 is refused"""
    h, W, _, _ = ectx
    rng = np.random.default_rng(size)
    c = np.stack([np.full(size, SAT, np.uint32), o.rand_elems(rng, size)])
    cv = val(c)
    kk = max(size.bit_length() - 1, 0)
    pts = [(0, 0, 0, 0), (1, 0, 0, 0), (F.root(kk), 0, 0, 0), tuple(int(v) for v in rng.integers(0, P, 4))]
    which = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.uint32)
    xs = np.stack([F.ext_to_mont(z) for z in pts + pts])
    got = h.batch_evaluate_any(h.copy_from_elem(c), 2, size, which, xs)
    for e in range(8):
        assert ext_val(got[e]) == F.vhorner_base(cv[which[e]], (pts + pts)[e], W), e
    if size > 2:   # size + 1 words of the first polynomial are in the buffer; the size is refused before any launch
        from raiko_amd._lib import RkError
        with pytest.raises(RkError):
            h.batch_evaluate_any(h.copy_from_elem(c), 1, size + 1, which[:1], xs[:1])


@pytest.mark.parametrize("count", [1, 16, 1 << 12])
def test_fri_folds_edges(ectx, count):
    h, W, gen, log_a = ectx
    rng = np.random.default_rng(count)
    A = 1 << log_a
    for data in ("saturated", "random"):
        inp = np.full((4, A * count), SAT, np.uint32) if data == "saturated" else o.rand_elems(rng, (4, A * count))
        ev = np.full((2 * count, 4), SAT, np.uint32) if data == "saturated" else o.rand_elems(rng, (2 * count, 4))
        for mix in [(0, 0, 0, 0), (1, 0, 0, 0), (P - 1, 0, 0, 0), tuple(int(v) for v in rng.integers(0, P, 4))]:
            out = h.alloc_elem(4 * count)
            h.fri_fold(out, h.copy_from_elem(inp), count, F.ext_to_mont(mix))
            want = F.fri_fold(val(inp), count, mix, log_a, W)
            assert np.array_equal(val(out.to_host()).reshape(4, count), want), (data, mix)
            oe = h.alloc_elem(4 * count)
            h.fri_fold_evals(oe, h.copy_from_elem(ev), count, F.ext_to_mont(mix))
            want = F.fri_fold_evals(val(ev), mix, W, gen)
            assert np.array_equal(val(oe.to_host()).reshape(count, 4), want), (data, mix)


def test_mix_and_sum_saturated(ectx):
    h, W, _, _ = ectx
    count = (1 << 12) + 5
    per_combo = [0, 1, 7, 8, 9, 17]
    combos = np.array([c for c, m in enumerate(per_combo) for _ in range(m)], np.uint32)
    combos = combos[np.random.default_rng(3).permutation(combos.size)]
    inp = np.full((combos.size, count), SAT, np.uint32)
    out0 = np.full((len(per_combo), count, 4), SAT, np.uint32)
    ms = mx = np.full(4, SAT, np.uint32)
    out = h.copy_from_elem(out0)
    h.mix_poly_coeffs(out, ms, mx, h.copy_from_elem(inp), combos, combos.size, count)
    want = F.mix_sum(val(out0), ext_val(ms), ext_val(mx), val(inp), combos, W)
    assert np.array_equal(val(out.to_host()).reshape(want.shape), want)
    for to_add in (1, 5, 33):
        e = np.full((to_add, count, 4), SAT, np.uint32)
        s = h.alloc_elem(4 * count)
        h.eltwise_sum_extelem(s, h.copy_from_elem(e), count, to_add)
        assert np.array_equal(val(s.to_host()), np.full(4 * count, to_add * VSAT % P, np.uint64))


@pytest.mark.parametrize("count", [2049, (1 << 20) + 3])
def test_prefix_products_edges(ectx, count):
    h, W, _, _ = ectx
    lib = h._lib
    a = (SAT, SAT, SAT, SAT)
    av = ext_val(a)
    # all-saturated elements: a^(i+1); then the same with one zero element in the middle
    want = F.ext_powers(av, count + 1, W)[1:]
    x = np.tile(np.array(a, np.uint32), (count, 1))
    buf = h.copy_from_elem(x)
    h._ck(lib.rk_prefix_products(h._ctx, buf.ptr, count))
    assert np.array_equal(val(buf.to_host()).reshape(count, 4), want)
    mid = count // 2
    x[mid] = 0
    buf = h.copy_from_elem(x)
    h._ck(lib.rk_prefix_products(h._ctx, buf.ptr, count))
    w2 = want.copy()
    w2[mid:] = 0
    assert np.array_equal(val(buf.to_host()).reshape(count, 4), w2)


@pytest.mark.parametrize("Hh", [4, 1 << 14])
@pytest.mark.parametrize("w", [1, 7, 8, 9, 31, 32, 33])
def test_pcs_open_and_reduce_saturated(ectx, Hh, w):
    """all-(p-1) matrices: the opened value of a constant column is that constant.  Reduce openings row-major and
    column-major (a constant matrix is the same words in either layout) with opened values that are NOT the true
    ones -- zeros, saturated words, random values -- so every numerator (row dot product minus opened dot product) is
    nonzero and the coefficient, the denominator x_r - z_j and the saturated sum into ro are all compared"""
    h, W, gen, _ = ectx
    p = h.get_params()
    blow, shift = int(p.blowup_log2), int(p.coset_shift)
    assert Hh >> blow >= 1, "the LDE must hold at least one row of the trace"
    rng = np.random.default_rng(w + Hh)
    lde = np.full((Hh, w), SAT, np.uint32)
    d_lde = h.copy_from_elem(lde)
    pts = [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(7)] + [(0, 0, 0, 0)]
    pm = np.stack([F.ext_to_mont(z) for z in pts])
    want_y = np.full((w, 4), 0, np.uint64)
    want_y[:, 0] = VSAT
    for npts in (1, 2, 3, 4):
        got = h.pcs_eval_at_many(d_lde, Hh, w, pm[:npts])
        gotc = h.pcs_eval_at_many_cols(d_lde, Hh, w, pm[:npts])
        for j in range(npts):
            assert np.array_equal(val(got[j]), want_y), (npts, j)
            assert np.array_equal(val(gotc[j]), want_y), (npts, j)
    assert np.array_equal(val(h.pcs_eval_at(d_lde, Hh, w, pm[0])), want_y)
    alpha = np.full(4, SAT, np.uint32)
    ro0 = np.full((Hh, 4), SAT, np.uint32)
    opened = {"zero": np.zeros((8, w, 4), np.uint32), "saturated": np.full((8, w, 4), SAT, np.uint32),
              "random": o.rand_elems(rng, (8, w, 4))}
    for yname, ys in opened.items():
        for npts in (1, 4, 8):
            want = F.pcs_reduce_openings(val(ro0), val(lde), Hh, pts[:npts], val(ys[:npts]),
                                         ext_val(alpha), 3, shift, gen, W)
            assert not np.array_equal(want, val(ro0)), "the numerators must not vanish"
            d_ro = h.copy_from_elem(ro0)
            h.pcs_reduce_openings(d_ro, d_lde, Hh, w, pm[:npts], ys[:npts], alpha, 3)
            assert np.array_equal(val(d_ro.to_host()).reshape(Hh, 4), want), (yname, npts)
            d_rc = h.copy_from_elem(ro0)
            h.pcs_reduce_openings_cols(d_rc, d_lde, Hh, w, pm[:npts], ys[:npts], alpha, 3)
            assert np.array_equal(val(d_rc.to_host()).reshape(Hh, 4), want), (yname, npts)
