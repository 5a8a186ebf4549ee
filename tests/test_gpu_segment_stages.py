"""rk_prove_segment as a run of stages (prover.hip, SegmentRun): a proof that ends early -- refused before its first
device call, or stopped by a failing hook with work queued -- leaves nothing in flight, so the next proof on the same
context is the oracle's word for word; and the stages are still charged to the rk_timing slots they always were."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as o
from raiko_amd import _lib
from raiko_amd.hal import make_c_segment
from raiko_amd.segment import Segment, make_tapset, synthetic_segment

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain():
    seg = synthetic_segment(5, (2, 2, 3), seed=505)
    return seg, o.oracle_prove(seg)


def prove_status(hal, seg):
    """rk_prove_segment itself, past the wrapper's own shape check: (status, seal words written)"""
    c_seg, keep = make_c_segment(seg)
    cap = int(hal._lib.rk_seal_bound_words(C.byref(c_seg)))
    assert cap > 0
    seal = np.zeros(cap, dtype=np.uint32)
    words = C.c_size_t(0)
    st = hal._lib.rk_prove_segment(hal._ctx, C.byref(c_seg), seal.ctypes.data_as(_lib.u32p), cap, C.byref(words))
    del keep
    return st, seal[: words.value]


def test_three_taps_on_two_rows_are_refused_up_front(hal, plain):
    """po2 = 1 and a register read at three rows: its interpolating polynomial has more coefficients than the segment
    has rows.  The tap set itself is well formed, so the seal bound accepts it and the prover must refuse."""
    rng = np.random.default_rng(41)
    taps = make_tapset([[(0, 1)], [(0,)], [(0,), (0, 1, 2)]])
    seg = Segment(po2=1, taps=taps, groups=[o.rand_elems(rng, (w, 2)) for w in (1, 1, 2)], check=o.rand_elems(rng, (4, 8)),
                  globals_=o.rand_elems(rng, (3,)), n_accum_mix=2)
    st, _ = prove_status(hal, seg)
    assert st == _lib.RK_ERR_INVALID
    ordinary, want = plain
    assert np.array_equal(hal.prove_segment(ordinary), want)


def test_proof_after_a_failing_accumulate_hook(hal, plain):
    """the hook fails after code and data were committed and with the accum buffer allocated: RK_ERR_CALLBACK, and the
    context proves the next segment as if nothing had happened"""
    seg = synthetic_segment(5, (2, 2, 3), seed=506)
    calls = []

    def accumulate(user, view, d_accum):
        calls.append(view.contents.po2)
        return 1

    hooks = _lib.RkCircuitHooks()
    hooks.accumulate = _lib.ACCUMULATE_FN(accumulate)
    seg.hooks = C.addressof(hooks)
    st, _ = prove_status(hal, seg)
    assert st == _lib.RK_ERR_CALLBACK and calls == [5]
    ordinary, want = plain
    assert np.array_equal(hal.prove_segment(ordinary), want)
    seg.hooks = None
    assert np.array_equal(hal.prove_segment(seg), o.oracle_prove(seg))


def test_every_stage_is_charged_to_its_slot(hal):
    """one po2 = 9 proof with a circuit behind the hooks (one FRI round): every slot of rk_timing gets device time --
    ntt and hash from the four commitments, circuit from the hooks, deep, fri, query -- and the outermost bracket,
    `total`, covers each of them"""
    from raiko_amd import toy_circuit
    toy_circuit.load()
    seg = toy_circuit.toy_segment(9, (8, 4, 8), seed=909)
    hal.prove_segment(seg)
    t = hal.last_timing()
    stages = ("ntt", "hash", "circuit", "deep", "fri", "query")
    assert set(t) == set(stages) | {"total"}
    for name in stages:
        assert t[name] > 0, (name, t)
    assert t["total"] >= max(t[name] for name in stages), t
