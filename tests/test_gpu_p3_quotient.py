"""rk_p3_prove with quotients in 4, 8 and 16 chunks (log_quotient_degree 2 to 4, blow-ups 4 to 16): the selector and
1 / Z_H tables indexed at i & (2^blowup - 1), the split of the quotient values into chunks (point i -> chunk i mod qd,
row i / qd) in the interpreter and in the hiprtc-generated kernel, the chunk shifts w_(n qd)^(-j i) and the chunk
matrices of one MMCS batch.  Every proof is compared with the oracle (the parametrized test of tests/test_gpu_p3.py
covers the seeded cases under the interpreter) and with the exact reference of tests/p3_ref.py."""
import json
import os

import numpy as np
import pytest

import oracle_lib as o
import p3_ref as R
from p3_cases import P3_CASES, REF_CASES, _AIRS, air_of, init_of, power_trace, sha, shapes, tables_of
from raiko_amd import hal as H, p3

pytestmark = pytest.mark.gpu
P = o.P
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "p3_digests.json")))
HIGH = sorted(c for c in P3_CASES if any(lqd >= 2 for _, lqd, _ in shapes(c)))        # the seeded cases of 4 chunks or more


def _blowup(preset, over):
    return over.get("blowup_log2", H.make_params(preset).blowup_log2)


@pytest.fixture()
def hal():
    R.p2_tables(0)
    R.p2_tables(1)
    h = H.HipHal(0)
    yield h
    o.oracle_set_params()
    h.close()
    _AIRS.clear()           # a compiled list stays compiled for the life of its handle: fresh AIR objects for the next test


@pytest.mark.parametrize("case", HIGH)
def test_generated_kernel_gives_the_committed_digest(hal, case):
    preset, over, _, _ = P3_CASES[case]
    blob = hal.set_params(preset, **over)
    _AIRS.clear()
    tables, init = tables_of(case), init_of(case)
    interp = p3.prove(hal, tables, init)
    for t in tables:
        t.air.compile(hal)          # rk_air_compile: straight-line HIP through hiprtc
    jit = p3.prove(hal, tables, init)
    assert {"words": int(jit.size), "sha256": sha(jit)} == GOLD[case]
    assert np.array_equal(interp, jit)
    assert p3.verify(tables, jit, init, params=blob) == 0


@pytest.mark.parametrize("case", REF_CASES)
def test_exact_reference_matches_the_gpu_proof(hal, case):
    """transcript, trace openings, quotient chunks and the zps recombination of tests/p3_ref.py against the GPU's proof
    words, interpreter and generated kernel; tables with lookups: their cumulative sums, permutation openings and
    quotients as well (tests/test_gpu_p3_lookups.py runs those cases under the generated kernel too)"""
    preset, over, _, _ = P3_CASES[case]
    hal.set_params(preset, **over)
    o.oracle_set_params(preset, **over)          # the Merkle-path case builds its chip rows under the case's parameter set
    tables, init = tables_of(case), init_of(case)
    R.check_proof(preset, _blowup(preset, over), tables, init, p3.prove(hal, tables, init))
    if case in HIGH:
        for t in tables:
            t.air.compile(hal)
        R.check_proof(preset, _blowup(preset, over), tables, init, p3.prove(hal, tables, init))


def test_device_resident_traces_at_every_lqd(hal):
    """lqd 0 .. 4 in one proof from traces already on the device, interpreter and generated kernel: the committed
    digest, and the inputs are left untouched"""
    case = "sp1_blow4_lqd0_to_4"
    preset, over, _, _ = P3_CASES[case]
    hal.set_params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    bufs = [hal.copy_from_elem(t.trace) for t in tables]
    dev = [(H._ptr(b), t.log_height) for b, t in zip(bufs, tables)]
    assert sha(p3.prove(hal, tables, init, device_traces=dev)) == GOLD[case]["sha256"]
    for t in tables:
        t.air.compile(hal)
    assert sha(p3.prove(hal, tables, init, device_traces=dev)) == GOLD[case]["sha256"]
    for b, t in zip(bufs, tables):
        assert np.array_equal(b.to_host().reshape(t.trace.shape), t.trace)


def test_shards_of_mixed_lqd_give_the_same_proofs(hal):
    """rk_p3_prove_shards at blow-up 16 over shards of lqd 2, 3 and 4 tables: `batch` 1 and 3 give the proofs of
    one-at-a-time proving, in order; a shard whose degree-17 transition is broken is reported by its index"""
    from raiko_amd._lib import RkError
    over = dict(queries=4, pow_bits=3, blowup_log2=4)
    blob = hal.set_params(1, **over)
    degs = (5, 9, 17)
    shards = []
    for i in range(6):
        tabs = [p3.Table.from_canonical(air_of("power", degs[(i + j) % 3]), *power_trace(2 + (i + 2 * j) % 5, degs[(i + j) % 3], seed=90 + 3 * i + j))
                for j in range(1 + i % 3)]
        shards.append((tabs, p3.to_mont([i, 5])))
    want = [p3.prove(hal, tables, init) for tables, init in shards]
    for batch in (1, 3):
        got = p3.prove_shards(shards, blob, batch=batch, verify=True)
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    o.oracle_set_params(1, **over)
    assert np.array_equal(want[5], o.oracle_p3_prove(*shards[5]))
    bad = list(shards)
    bad[4] = ([p3.Table.from_canonical(air_of("power", 17), *power_trace(4, 17, seed=5, kick_row=3))], p3.to_mont([4]))
    with pytest.raises(RkError) as ei:
        p3.prove_shards(bad, blob, batch=3, verify=True)
    assert ei.value.status == -7 and ei.value.segment == 4
    assert len(p3.prove_shards(bad, blob, batch=3, verify=False)) == 6
    H.session_release()


@pytest.mark.parametrize("preset", [0, 1])
@pytest.mark.parametrize("D", [5, 9, 17])
def test_broken_trace_proof_equals_the_oracle_and_is_refused(hal, preset, D):
    """lqd 2, 3, 4 at blow-up 16, interpreter and generated kernel: a trace whose degree-D transition fails once gives
    the oracle's proof words, both verifiers refuse it with reason 3, and the exact reference reproduces its chunks"""
    over = dict(queries=3, pow_bits=2, blowup_log2=4)
    blob = hal.set_params(preset, **over)
    o.oracle_set_params(preset, **over)
    air = air_of("power", D)
    bad = [p3.Table.from_canonical(air, *power_trace(6, D, seed=80 + D, kick_row=21))]
    init = p3.to_mont([preset, D])
    want = o.oracle_p3_prove(bad, init)
    for compiled in (False, True):
        if compiled:
            air.compile(hal)
        pf = p3.prove(hal, bad, init)
        assert np.array_equal(pf, want), compiled
    assert p3.verify(bad, pf, init, params=blob) == 3 == o.oracle_p3_verify(bad, pf, init)
    with pytest.raises(AssertionError, match="zps recombination"):
        R.check_proof(preset, 4, bad, init, pf)
