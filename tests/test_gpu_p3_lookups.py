"""The lookup half of rk_p3_prove against the exact reference of tests/p3_ref.py (plain integers and numpy, nothing of the
oracle), at the sizes where its kernels change behaviour: perm_entries_kernel (256 rows per workgroup, the staging's clamp
below that, two staged columns per lane, the 120-column cap, the raised dynamic-LDS attribute from 64 used columns on),
psum_totals / psum_carry / psum_apply (blocks of 2048 rows; one carry workgroup whose lanes take ceil(blocks / 256) totals
each: 1 up to 2^19 rows, 2 at 2^20), the cumulative sums, the permutation openings at zeta and zeta g, and the quotient of
tables with interactions (taps on permutation columns, challenge and cumulative-sum leaves, PERM_NEXT wrapping) under the
interpreter and the hiprtc-generated kernel.

Every proof is judged by R.check_proof word for word (dense quotient where log_n + lqd <= 12, the O(n) mode above), the
generated kernel must give the interpreter's words, p3.verify returns 0 for balanced tables and 8 for their unbalanced
twins, and proofs of tables up to 2^14 rows are also the oracle's words.  The edge tables are tests/p3_lookup_cases.py's;
its asserts (no zero prefix of the running sum, no all-zero batch, the edge multiplicities present) are repeated on the
permutation trace of every proof, under the proof's own challenges.

Wall time on an MI355X host: the 2^19 / 2^20 test takes 5.5 s (5.0 s of it the host reference), test_full_size_tables of
tests/test_gpu_p3.py 30.7 s in the same run; every other case takes about 3 s or less."""
import time

import numpy as np
import pytest

import oracle_lib as o
import p3_lookup_cases as LC
import p3_ref as R
from p3_cases import P3_CASES, REF_CASES, _AIRS, init_of, shapes, tables_of
from raiko_amd import hal as H, p3

pytestmark = pytest.mark.gpu
P = o.P
OVER = dict(queries=3, pow_bits=1)
LOOKUP_REF_CASES = [c for c in REF_CASES if any(perm for _, _, perm in shapes(c))]


@pytest.fixture()
def hal():
    R.p2_tables(0)                  # the presets' Poseidon2 constants, read before any parameter set changes
    R.p2_tables(1)
    _AIRS.clear()
    LC._EDGE_AIRS.clear()
    h = H.HipHal(0)
    yield h
    o.oracle_set_params()
    h.close()
    _AIRS.clear()                   # a compiled list stays compiled for the life of its handle
    LC._EDGE_AIRS.clear()


def _sp1(hal):
    o.oracle_set_params(1, **OVER)
    return hal.set_params(1, **OVER)


def _prove_both_ways(hal, jobs):
    """jobs = [(tables, init)] -> their proofs.  Every job under the interpreter first, in order; then every AIR compiled
    (rk_air_compile) and every job again, in the same order: the same words"""
    interp = [p3.prove(hal, tables, init) for tables, init in jobs]
    for tables, _ in jobs:
        for t in tables:
            t.air.compile(hal)
    for k, ((tables, init), want) in enumerate(zip(jobs, interp)):
        assert np.array_equal(p3.prove(hal, tables, init), want), "job %d: generated kernel against interpreter" % k
    return interp


def _judge(blob, tables, init, pf, verdict, preset=1, blowup_log2=1):
    tall = any(t.log_height + t.air.log_quotient_degree() > 12 for t in tables)
    seen = {}
    R.check_proof(preset, blowup_log2, tables, init, pf, tall=tall, perm_out=seen)
    assert sorted(seen) == [i for i, t in enumerate(tables) if t.air.perm_width]
    for ti, pt in seen.items():
        if hasattr(tables[ti], "edge"):
            LC.assert_edges(tables[ti], pt)
    assert p3.verify(tables, pf, init, params=blob) == verdict
    if max(t.log_height for t in tables) <= 14:
        assert np.array_equal(pf, o.oracle_p3_prove(tables, init)), "the oracle's words"
    return seen


@pytest.mark.parametrize("case", LOOKUP_REF_CASES)
def test_seeded_lookup_cases_in_full_under_both_evaluators(hal, case):
    """every seeded case with interactions (2 to 2^9 rows, 1 to 7 interactions, both presets, lqd up to 3, the Poseidon2
    chip beside the Merkle-path table): cumulative sums, all permutation openings and all quotient chunks are the exact
    reference's, from the interpreter and from the generated kernel"""
    preset, over, _, _ = P3_CASES[case]
    blob = hal.set_params(preset, **over)
    o.oracle_set_params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf, = _prove_both_ways(hal, [(tables, init)])
    seen = _judge(blob, tables, init, pf, 0, preset, over.get("blowup_log2", H.make_params(preset).blowup_log2))
    assert seen


@pytest.mark.parametrize("log_n", [1, 7, 8, 9, 11, 12])
def test_heights_around_the_workgroup_and_the_prefix_sum_block(hal, log_n):
    """three interactions (a last batch of one) at 2 and 128 rows (less than one perm_entries workgroup: the staging clamps
    its loads to row n - 1), 256 (exactly one), 512 (two); 2048 rows (one full psum block: no carry to add) and 4096 (two:
    the first height at which psum_apply adds a carried total); all below 2048 are partial psum blocks.  Balanced table
    and unbalanced twin"""
    blob = _sp1(hal)
    init = p3.to_mont([log_n])
    twins = [LC.edge_table(log_n, 3, 7, seed=20 + log_n, unbalanced=u) for u in (False, True)]
    proofs = _prove_both_ways(hal, [([t], init) for t in twins])
    for t, pf, verdict in zip(twins, proofs, (0, 8)):
        _judge(blob, [t], init, pf, verdict)


def test_used_column_boundaries_in_one_context(hal):
    """63, 64, 65 and 120 used columns at 512 rows, then 1: lanes 0..63 stage one column each up to 64, the second load
    per lane starts at 65, 120 is the cap; from 64 columns on the tile (n_used x 257 words: 65 792 bytes) needs the raised
    dynamic-LDS attribute, which stays on the function -- the 1-column launch after the 120-column one (twice: interpreter
    pass and generated-kernel pass) must still be right.  The 120-column table and the 1-column table with their twins"""
    blob = _sp1(hal)
    init = p3.to_mont([9, 120])
    shapes_ = [(3, 63, False), (2, 64, False), (3, 65, False), (2, 120, False), (2, 120, True), (1, 1, False), (1, 1, True)]
    tabs = [LC.edge_table(9, L, n_used, seed=30, unbalanced=u) for L, n_used, u in shapes_]
    used = lambda air: {c for it in air.interactions for c in it.value_cols} | {it.mult for it in air.interactions if not it.mult_is_const}
    assert [len(used(t.air)) for t in tabs] == [s[1] for s in shapes_]
    proofs = _prove_both_ways(hal, [([t], init) for t in tabs])
    for t, pf, (_, _, u) in zip(tabs, proofs, shapes_):
        _judge(blob, [t], init, pf, 8 if u else 0)


@pytest.mark.parametrize("L,n_used", [(1, 1), (1, 65), (2, 6), (16, 8)])
def test_interaction_counts(hal, L, n_used):
    """1, 2 and 16 interactions at 256 rows: a single batch of one (with no value at all, and with the longest tuple
    there is: 64 values), one full batch, eight batches (multiplicities from a column and from the constants 1 and p - 1,
    sends and receives in both positions of a batch).  Balanced table and unbalanced twin"""
    blob = _sp1(hal)
    init = p3.to_mont([L, n_used])
    twins = [LC.edge_table(8, L, n_used, seed=40, unbalanced=u) for u in (False, True)]
    if L == 16:
        its = twins[0].air.interactions
        assert {(it.mult_is_const, it.mult) for it in its if it.mult_is_const} == {(True, 1), (True, P - 1)}
        assert {(i % 2, it.kind) for i, it in enumerate(its)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    proofs = _prove_both_ways(hal, [([t], init) for t in twins])
    for t, pf, verdict in zip(twins, proofs, (0, 8)):
        _judge(blob, [t], init, pf, verdict)


def test_the_carry_pass_with_one_and_two_totals_per_lane(hal):
    """psum_carry_kernel: 2^19 rows are 256 block totals (one per lane, every lane busy), 2^20 rows are 512 (two per lane:
    the smallest height at which the lane's `for (i = lo; i < hi; i++)` walk runs twice).  Two interactions over six
    columns, balanced table and unbalanced twin at both heights, the balanced ones also from a device-resident trace; the
    reference in its O(n) mode: transcript, trace openings, cumulative sums, all permutation openings.

    Wall time measured on an MI355X host (one run): this test 5.5 s, of which the host reference and verifier 5.0 s and
    all the proving 0.1 s; tests/test_gpu_p3.py::test_full_size_tables in the same run: 30.7 s.  The reference part stays
    well below that yardstick, so both twins are kept at 2^19 too."""
    blob = _sp1(hal)
    init = p3.to_mont([19, 20])
    t_gpu = t_ref = 0.0
    for log_n in (19, 20):
        twins = [LC.edge_table(log_n, 2, 6, seed=50 + log_n, unbalanced=u, check=False) for u in (False, True)]
        t0 = time.perf_counter()
        proofs = _prove_both_ways(hal, [([t], init) for t in twins])
        buf = hal.copy_from_elem(twins[0].trace)
        assert np.array_equal(p3.prove(hal, [twins[0]], init, device_traces=[(H._ptr(buf), log_n)]), proofs[0])
        assert np.array_equal(buf.to_host().reshape(twins[0].trace.shape), twins[0].trace)      # left untouched
        del buf
        t1 = time.perf_counter()
        for t, pf, verdict in zip(twins, proofs, (0, 8)):
            seen = _judge(blob, [t], init, pf, verdict)
            assert bool(np.any(seen[0][-1, -4:])) == (verdict == 8)
        t_gpu, t_ref = t_gpu + t1 - t0, t_ref + time.perf_counter() - t1
    print("carry pass: proving %.1f s, host reference and verifier %.1f s" % (t_gpu, t_ref))


def test_four_tables_whose_cumulative_sums_cancel(hal):
    """p3.lookup_demo_tables(12, 8): cpu, add and mul tables of 2^12 rows (two psum blocks each) and a range table of 2^8
    in one proof under shared challenges: every table's cumulative sum is nonzero and the reference's, and they add up to
    zero"""
    blob = _sp1(hal)
    init = p3.to_mont([12, 8])
    tables = p3.lookup_demo_tables(12, 8, seed=7, airs=p3.lookup_demo_airs())
    assert [t.log_height for t in tables] == [12, 12, 12, 8]
    pf, = _prove_both_ways(hal, [(tables, init)])
    seen = _judge(blob, tables, init, pf, 0)
    sums = R.parse(tables, pf)["cumsums"]
    assert len(sums) == 4 and all(any(s) for s in sums)
    assert [sum(s[k] for s in sums) % P for k in range(4)] == [0, 0, 0, 0]
    assert [[int(v) for v in seen[i][-1, -4:]] for i in range(4)] == sums
