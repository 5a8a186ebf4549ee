"""The DEEP stage's streaming kernels, eval_dot_kernel and mix_kernel, after their move to lazy 64-bit accumulation
(raiko_amd/csrc/poly_lazy.hpp), through the HAL entry points and against the exact reference of tests/field_ref.py,
word for word.

eval_dot_kernel runs DOT_BLOCKS * TPB = 64 * 256 = 2^14 lanes per evaluation, lane l taking the terms l, l + 2^14, ...,
and folds its accumulators after every FOLD_TERMS = 4 terms.  rk_batch_evaluate_any takes powers of two only, so a
lane sees size / 2^14 terms, itself a power of two: at sizes 1 and 2 one or two lanes see a single term, at 2^14 every
lane sees one term (the remainder loop alone), and at 2^18 = 2^14 * 4 * 4 every lane passes four fold intervals.  A
lane that folds at least twice AND has a remainder needs 9 or more terms that are no multiple of 4, which no power of
two gives: that combination is covered on the host by tests/test_poly_lazy_host.py (1 000 and FOLD_TERMS + 1 terms).
The evaluations of one call go to batches of 8, 4, 2 and 1 per power table, so the counts 1, 7, 8, 9 and 17 with one
and three points take every batch width, alone and mixed.

The entry point builds its power tables itself, so the table cannot be filled with p - 1 directly; the saturated set
uses the point -1, whose powers are +-1, on coefficients that are all the raw word p - 1 (the host test carries the
all-(p - 1) table)."""
import numpy as np
import pytest

import field_ref as F
import oracle_lib as o
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

P = F.P
SAT = P - 1                      # raw word
DOT_LANES = 64 * 256             # DOT_BLOCKS * TPB of kernels_poly.hip
FOLD_TERMS = 4                   # pl::FOLD_TERMS of poly_lazy.hpp
SIZE_FOLDS = DOT_LANES * FOLD_TERMS * 4
N_COLS = 17


def val(words):
    words = np.asarray(words)
    assert (words < P).all(), "non-canonical word %d" % int(words.max())
    return F.from_mont(words)


@pytest.fixture(scope="module", params=[0, 1], ids=["risc0", "sp1"])
def ctx(request):
    h = H.HipHal(0)
    h.set_params(preset=request.param)
    yield h, (F.W_RISC0 if request.param == 0 else F.W_SP1)
    h.close()


_EVAL_SETS = {}


def eval_set(size, data, W):
    """(raw coefficient words (N_COLS, size), three points, reference value per (column, point)), built once"""
    key = (size, data, W)
    if key not in _EVAL_SETS:
        rng = np.random.default_rng(size * 2 + (data == "random"))
        if data == "random":
            c = o.rand_elems(rng, (N_COLS, size))
            pts = [tuple(int(v) for v in rng.integers(0, P, 4)) for _ in range(3)]
        else:
            c = np.full((N_COLS, size), SAT, np.uint32)
            pts = [(P - 1, 0, 0, 0), tuple(int(v) for v in rng.integers(0, P, 4)), (P - 1, P - 1, P - 1, P - 1)]
        cv = val(c)
        tables = [F.ext_powers(x, size, W) for x in pts]
        ref = {(col, j): tuple(int(v) for v in F.vmul(tables[j], cv[col][:, None]).sum(axis=0) % P)
               for col in range(N_COLS) for j in range(3)}
        _EVAL_SETS[key] = (c, pts, ref)
    return _EVAL_SETS[key]


def eval_patterns(n):
    """(name, column per evaluation, point index per evaluation)"""
    e = np.arange(n)
    return [("one point", e % N_COLS, np.zeros(n, int)),
            ("three points interleaved", e % N_COLS, e % 3),
            ("one column at three points", np.full(n, 5), e % 3),
            ("repeated pairs", (e // 2) % N_COLS, (e // 2) % 2)]


@pytest.mark.parametrize("data", ["random", "saturated"])
@pytest.mark.parametrize("size", [1, 2, DOT_LANES, SIZE_FOLDS])
def test_batch_evaluate_any_batches(ctx, size, data):
    h, W = ctx
    c, pts, ref = eval_set(size, data, W)
    xs_m = np.stack([F.ext_to_mont(x) for x in pts])
    buf = h.copy_from_elem(c)
    for n in (1, 7, 8, 9, 17):
        for name, which, sel in eval_patterns(n):
            got = h.batch_evaluate_any(buf, N_COLS, size, which.astype(np.uint32), xs_m[sel])
            for e in range(n):
                assert tuple(int(v) for v in val(got[e])) == ref[(int(which[e]), int(sel[e]))], (name, n, e)
    buf.free()


def combo_patterns(w):
    return [("all one", np.zeros(w, np.uint32)),
            ("alternating two", (np.arange(w) % 2).astype(np.uint32)),
            ("one column alone", np.array([1 if i == w // 2 else 0 for i in range(w)], np.uint32))]


@pytest.mark.parametrize("data", ["random", "saturated"])
@pytest.mark.parametrize("count", [1, 64, 1 << 12])
def test_mix_poly_coeffs_columns_and_combos(ctx, count, data):
    """the public call accumulates: `out` starts non-zero (random or saturated words) and a combo that no column
    names keeps its words"""
    h, W = ctx
    rng = np.random.default_rng(count)
    for w in (1, 7, 8, 9, 33):
        if data == "random":
            inp = o.rand_elems(rng, (w, count))
            out0 = o.rand_elems(rng, (2, count, 4))
            ms, mx = o.rand_elems(rng, 4), o.rand_elems(rng, 4)
        else:
            inp = np.full((w, count), SAT, np.uint32)
            out0 = np.full((2, count, 4), SAT, np.uint32)
            ms = mx = np.full(4, SAT, np.uint32)
        dev_in = h.copy_from_elem(inp)
        for name, combos in combo_patterns(w):
            out = h.copy_from_elem(out0)
            h.mix_poly_coeffs(out, ms, mx, dev_in, combos, w, count)
            want = F.mix_sum(val(out0), tuple(int(v) for v in val(ms)), tuple(int(v) for v in val(mx)), val(inp), combos, W)
            assert np.array_equal(val(out.to_host()).reshape(want.shape), want), (name, w)
            out.free()
        dev_in.free()
