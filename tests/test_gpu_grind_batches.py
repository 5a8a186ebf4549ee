"""Entry points past their first launch, against the oracle, exactly.

rk_pow_grind / rk_duplex_grind try 2^max(16, bits + 2) candidates per launch and launch again, from `base` = the number
tried so far, when none of them hit.  At 14 bits a batch of 2^16 holds no hit with probability e^-4: the seeds of
threshold_cases.GRIND_SEEDS are such inputs (tests/test_launch_thresholds.py checks, with the oracle's literal search,
that every nonce lies in the second batch), for both grinds and all four Poseidon2 instances; one ordinary seed per
instance keeps the first launch beside them.

rk_scatter launches at most 16384 workgroups of 256 lanes; past that many entries both of its kernels loop with the
grid's stride.  The case has 1000 entries more, each of them a second write to a word an entry of the first pass wrote
-- by the same lane or by a lane of another workgroup -- and the result is or_scatter's, word for word."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as o
import p2_edges as E
import threshold_cases as T
from raiko_amd import _lib
from raiko_amd.hal import HipHal

pytestmark = pytest.mark.gpu


@pytest.fixture()
def cfg():
    """a context of its own and the oracle under one blob; both back to risc0's defaults afterwards"""
    h = HipHal(0)

    def apply(w, m4):
        preset, kw = T.grind_params(w, m4)
        o.oracle_set_params(preset, **kw)
        return h.set_params(preset, **kw)

    yield h, apply
    h.close()
    o.oracle_set_params()


def gpu_pow_grind(h, cells, bits):
    nonce = C.c_uint32(0)
    _lib.check(h._ctx, h._lib.rk_pow_grind(h._ctx, cells.ctypes.data_as(_lib.u32p), bits, C.byref(nonce)))
    return nonce.value


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_duplex_grind_hits_in_the_second_launch(cfg, w, m4):
    h, apply = cfg
    apply(w, m4)
    for seed, nonce in T.GRIND_SEEDS[(w, m4)]["duplex"]:
        state, inputs = T.duplex_inputs(w, seed)
        assert nonce >= 1 << 16
        assert h.duplex_grind(state, inputs, T.GRIND_BITS) == nonce == T.oracle_duplex_grind(w, seed), seed
    seed = T.GRIND_FIRST_SEEDS["duplex"]
    want = T.oracle_duplex_grind(w, seed)
    assert want < 1 << 16 and h.duplex_grind(*T.duplex_inputs(w, seed), T.GRIND_BITS) == want


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_pow_grind_hits_in_the_second_launch(cfg, w, m4):
    h, apply = cfg
    apply(w, m4)
    for seed, nonce in T.GRIND_SEEDS[(w, m4)]["pow"]:
        assert nonce >= 1 << 16
        assert gpu_pow_grind(h, T.pow_cells(w, seed), T.GRIND_BITS) == nonce == T.oracle_pow_grind(w, seed), seed
    seed = T.GRIND_FIRST_SEEDS["pow"]
    want = T.oracle_pow_grind(w, seed)
    assert want < 1 << 16 and gpu_pow_grind(h, T.pow_cells(w, seed), T.GRIND_BITS) == want


def scatter(hal, buf, words, index, offsets, values):
    p = lambda a: a.ctypes.data_as(_lib.u32p)
    _lib.check(hal._ctx, hal._lib.rk_scatter(hal._ctx, buf.ptr, words, p(index), index.size - 1, p(offsets), p(values)))


def test_scatter_past_one_grid_the_last_write_wins(hal, orc):
    k = T.constants()
    index, offsets, values, start, _, _ = T.scatter_case(k)
    n = offsets.size
    assert n == T.scatter_entries(k) > k["SCATTER_GRID"] * k["SCATTER_TPB"]
    want = start.copy()
    orc.or_scatter(o.ptr(want), o.ptr(index), n, o.ptr(offsets), o.ptr(values))
    buf = hal.copy_from_elem(start)
    scatter(hal, buf, T.SCATTER_INTO, index, offsets, values)
    got = buf.to_host()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_scatter_every_entry_to_one_word(hal, orc):
    """5000 entries (20 workgroups) and one target: the last entry's value stays, everything else is untouched"""
    rng = np.random.default_rng(43)
    n, words, target = 5000, 300, 77
    index = np.arange(n + 1, dtype=np.uint32)
    offsets = np.full(n, target, dtype=np.uint32)
    values = o.rand_elems(rng, (n,))
    start = o.rand_elems(rng, (words,))
    want = start.copy()
    orc.or_scatter(o.ptr(want), o.ptr(index), n, o.ptr(offsets), o.ptr(values))
    assert want[target] == values[-1] and np.array_equal(np.delete(want, target), np.delete(start, target))
    buf = hal.copy_from_elem(start)
    scatter(hal, buf, words, index, offsets, values)
    assert np.array_equal(buf.to_host(), want)
