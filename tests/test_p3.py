"""Plonky3-style STARK, CPU side: the oracle (oracle/or_p3.c) against its own verifier, against the committed digests and
against the PRODUCT's host verifier rk_p3_verify (no GPU needed for verification), plus the AIR front end
(rk_air_create: validation, symbolic degree) and hostile proofs.  Reference call site of the path:
provers/sp1/driver/src/lib.rs:44-57 (`client.prove`); the Plonky3 crates are outside the reference tree -- RECALLED,
parity unpinned: what pins the oracle here is that an independent verifier written from the verifier's side of the
protocol (reduced openings recomputed from opened rows, folds as lines through (x, e), (-x, e')) accepts it and that
the constraint identity holds only for traces that satisfy their AIR."""
import json
import os

import numpy as np
import pytest

import oracle_lib as o
from p3_cases import P3_CASES, REF_CASES, init_of, sha, shapes, tables_of
from raiko_amd import _lib, hal, p3

P = o.P
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "p3_digests.json")))


@pytest.fixture()
def params():
    yield o.oracle_set_params
    o.oracle_set_params()


def test_cases_match_committed_digests_and_both_verifiers_accept(params):
    assert sorted(GOLD) == sorted(P3_CASES)
    for case, (preset, over, _, _) in P3_CASES.items():
        params(preset, **over)
        blob = hal.make_params(preset, **over)
        tables, init = tables_of(case), init_of(case)
        for t in tables:
            assert t.air.check_trace(o.from_mont(t.trace), o.from_mont(t.public_values)) == [] or t.trace.shape[0] > 256
        pf = o.oracle_p3_prove(tables, init)
        assert {"words": int(pf.size), "sha256": sha(pf)} == GOLD[case], case
        assert o.oracle_p3_verify(tables, pf, init) == 0
        assert p3.verify(tables, pf, init, params=blob) == 0
        arr, keep = p3._c_tables(tables)                  # rk_p3_proof_bound_words is exact (lookups or not)
        assert _lib.load().rk_p3_proof_bound_words(blob, arr, len(tables)) == pf.size, case
        # bound to the statement: other init words, other public values, another parameter set
        assert p3.verify(tables, pf, np.concatenate([init, [1]]).astype(np.uint32), params=blob) != 0
        if tables[0].public_values.size:
            other = p3.Table(tables[0].air, tables[0].trace, tables[0].public_values.copy())
            other.public_values[0] = (int(other.public_values[0]) + 1) % P
            assert p3.verify([other] + tables[1:], pf, init, params=blob) != 0
            assert o.oracle_p3_verify([other] + tables[1:], pf, init) != 0
        assert p3.verify(tables, pf, init, params=hal.make_params(1 - preset)) != 0


def test_symbolic_degree_and_info(params):
    lib = o.oracle()
    for name, arg, want in (("fib", None, 0), ("cubic", 6, 1), ("wide", 9, 1)):
        from p3_cases import air_of
        air = air_of(name, arg)
        steps = np.ascontiguousarray(air.steps, dtype=np.uint32)
        oair = o.OrAir(steps=steps.ctypes.data, n_steps=steps.shape[0])
        assert air.log_quotient_degree() == want == lib.or_air_log_quotient_degree(oair) == air.info()["log_quotient_degree"]
        assert air.info()["n_constraints"] == air.n_constraints
    # a degree-5 constraint needs four chunks; a degree-9 one more than any supported blow-up covers
    b = p3.AirBuilder(1)
    x = b.local(0)
    b.assert_zero(x * x * x * x * x - x)
    assert b.build().info()["log_quotient_degree"] == 2


def test_air_create_rejects_malformed_lists():
    lib = _lib.load()
    import ctypes as C

    def create(steps, width=2, n_public=1):
        a = np.array(steps, dtype=np.uint32).reshape(-1, 3)
        h = C.c_void_p()
        rc = lib.rk_air_create(a.ctypes.data, a.shape[0], width, n_public, C.byref(h))
        if rc == 0:
            lib.rk_air_destroy(h)
        return rc

    assert create([(p3.LOCAL, 0, 0), (p3.ASSERT_ZERO, 0, 0)]) == 0
    assert create([(p3.LOCAL, 2, 0), (p3.ASSERT_ZERO, 0, 0)]) == -1          # column out of range
    assert create([(p3.PUBLIC, 1, 0), (p3.ASSERT_ZERO, 0, 0)]) == -1         # public value out of range
    assert create([(p3.LOCAL, 0, 0), (p3.ADD, 0, 1), (p3.ASSERT_ZERO, 1, 0)]) == -1   # operand not yet pushed
    assert create([(p3.LOCAL, 0, 0), (p3.ASSERT_ZERO, 1, 0)]) == -1
    assert create([(p3.CONST, P, 0), (p3.ASSERT_ZERO, 0, 0)]) == -1          # not canonical
    assert create([(16, 0, 0)]) == -1                                        # unknown op
    for op in (p3.PERM_LOCAL, p3.PERM_NEXT, p3.CHALLENGE, p3.CUMSUM):       # leaves of a lookup argument the AIR does not have
        assert create([(op, 0, 0)]) == -1
    assert create([(p3.LOCAL, 0, 0)]) == 0                                   # no constraint at all is a valid (empty) AIR


def test_lookup_air_create_rejects_malformed_interactions():
    lib = _lib.load()
    import ctypes as C
    steps = np.array([(p3.LOCAL, 0, 0)], dtype=np.uint32)

    def create(words, n, width=3, steps=steps, ext_w=0):
        w = np.array(words, dtype=np.uint32)
        h = C.c_void_p()
        rc = lib.rk_air_create_lookup(steps.ctypes.data, steps.shape[0], width, 0, w.ctypes.data_as(_lib.u32p), n, w.size, ext_w, C.byref(h))
        if rc == 0:
            lib.rk_air_destroy(h)
        return rc

    assert create([0, 1, 1, 1, 2, 0, 1], 1) == 0
    assert create([2, 1, 1, 1, 2, 0, 1], 1) == -1            # kind
    assert create([0, P, 1, 1, 2, 0, 1], 1) == -1            # bus not canonical
    assert create([0, 1, 1, P, 2, 0, 1], 1) == -1            # constant multiplicity not canonical
    assert create([0, 1, 0, 3, 2, 0, 1], 1) == -1            # multiplicity column out of range
    assert create([0, 1, 1, 1, 2, 0, 3], 1) == -1            # value column out of range
    assert create([0, 1, 1, 1, 2, 0], 1) == -1               # short
    assert create([0, 1, 1, 1, 2, 0, 1, 0], 1) == -1         # trailing words
    assert create([0, 1, 1, 1, 65] + [0] * 65, 1) == -1      # tuple too long
    assert create([0, 1, 1, 1, 2, 0, 1], 2) == -1            # count and words disagree
    wide = [w for k in range(2) for w in [0, 1, 1, 1, 60] + list(range(60 * k, 60 * k + 60))]
    assert create(wide, 2, width=200) == 0                   # 120 distinct columns: the limit
    assert create(wide + [0, 1, 1, 1, 1, 120], 3, width=200) == -1
    # the permutation leaves are range-checked against what the interactions give: 1 interaction = 8 base columns,
    # a tuple of 2 = alpha, beta^0..beta^2 = 16 challenge words
    # random word lists: accepted or refused, never anything else (this file also runs under ASan / UBSan: tests/asan)
    rng = np.random.default_rng(5)
    seen = set()
    for k in range(400):
        n_ix = int(rng.integers(0, 5))
        words = []
        for _ in range(n_ix):
            nv = int(rng.integers(0, 5))
            words += [int(rng.integers(0, 3)), int(rng.integers(0, 9)), int(rng.integers(0, 3)), int(rng.integers(0, 5)), nv if rng.random() < 0.9 else nv + 1]
            words += [int(v) for v in rng.integers(0, 4, size=nv)]
        if rng.random() < 0.2 and words:
            words = words[: int(rng.integers(0, len(words)))]
        seen.add(create(words or [0], n_ix if words else 0, ext_w=int(rng.integers(0, 2)) * 11) if words or n_ix == 0 else -1)
    assert seen == {0, -1}
    for op, lim in ((p3.PERM_LOCAL, 8), (p3.PERM_NEXT, 8), (p3.CHALLENGE, 16), (p3.CUMSUM, 4)):
        ok = np.array([(op, lim - 1, 0)], dtype=np.uint32)
        bad = np.array([(op, lim, 0)], dtype=np.uint32)
        assert create([0, 1, 1, 1, 2, 0, 1], 1, steps=ok) == 0 and create([0, 1, 1, 1, 2, 0, 1], 1, steps=bad) == -1


def test_library_written_lookup_constraints_give_the_same_proofs(params):
    """rk_air_create_lookup with ext_w != 0 appends eval_permutation_constraints itself (a binding hands over the chip's
    own constraints and its interactions, nothing else): the same identities as AirBuilder writes, so the oracle's proof
    over either list is the same words"""
    import ctypes as C
    from p3_cases import EXT_W, selfperm_air, widetuple_air
    for preset in (0, 1):
        over = dict(queries=4, pow_bits=2)
        params(preset, **over)
        blob = hal.make_params(preset, **over)
        w = EXT_W[preset]

        def both(make, trace):
            b1, b2 = make(), make()
            a_py, a_lib = b1.build(), b2.build(library_constraints=True)
            assert a_lib.steps.shape[0] > len(b2.steps) and a_lib.n_constraints == a_py.n_constraints
            assert a_lib.info()["log_quotient_degree"] == a_py.info()["log_quotient_degree"] == a_py.log_quotient_degree()
            return p3.Table.from_canonical(a_py, trace), p3.Table.from_canonical(a_lib, trace)

        def cpu():
            b = p3.AirBuilder(5, 0, w)
            b.assert_zero(b.local(4) * (b.local(4) - 1))
            b.send(2, [0, 1, 2], mult=4, mult_is_const=False)
            b.send(3, [0, 1, 3], mult=4, mult_is_const=False)
            b.send(1, [0], mult=4, mult_is_const=False)
            return b

        def selfp():
            b = p3.AirBuilder(10, 0, w)
            for kind, bus, cols, m, const in ((0, 5, list(range(8)), 2, True), (1, 5, list(range(8)), 1, True), (1, 5, list(range(8)), 1, True),
                                              (0, 6, [3], 8, False), (1, 6, [3], 8, False), (0, 7, [], 5, True), (1, 7, [], 5, True)):
                (b.send if kind == 0 else b.receive)(bus, cols, mult=m, mult_is_const=const)
            return b

        rng = np.random.default_rng(preset)
        demo = p3.lookup_demo_tables(4, 3, seed=3, ext_w=w)
        t_py, t_lib = both(cpu, o.from_mont(demo[0].trace))
        s_py, s_lib = both(selfp, rng.integers(0, P, size=(16, 10)))
        init = p3.to_mont([preset])
        pf_py = o.oracle_p3_prove([t_py] + demo[1:] + [s_py], init)
        pf_lib = o.oracle_p3_prove([t_lib] + demo[1:] + [s_lib], init)
        assert np.array_equal(pf_py, pf_lib)
        assert p3.verify([t_lib] + demo[1:] + [s_lib], pf_py, init, params=blob) == 0
    # the caller's list may not name the permutation trace when the library writes those constraints; W must be canonical
    lib = _lib.load()
    h = C.c_void_p()
    iw = np.array([0, 1, 1, 1, 1, 0], dtype=np.uint32)
    for steps, ext_w, want in (([(p3.LOCAL, 0, 0)], 11, 0), ([(p3.PERM_LOCAL, 0, 0)], 11, -1), ([(p3.LOCAL, 0, 0)], P, -1)):
        a = np.array(steps, dtype=np.uint32)
        rc = lib.rk_air_create_lookup(a.ctypes.data, a.shape[0], 2, 0, iw.ctypes.data_as(_lib.u32p), 1, iw.size, ext_w, C.byref(h))
        assert rc == want
        if rc == 0:
            lib.rk_air_destroy(h)
    a = np.array([(p3.LOCAL, 0, 0)], dtype=np.uint32)
    assert lib.rk_air_create_lookup(a.ctypes.data, 1, 2, 0, None, 0, 0, 11, C.byref(h)) == -1      # W without interactions


@pytest.mark.parametrize("preset", [0, 1])
def test_lookups_that_do_not_balance_are_rejected_by_both_verifiers(params, preset):
    """the permutation argument's own failure modes: a multiplicity that is off by one, a tuple nobody receives
    (cumulative sums do not cancel: reason 8); cumulative sums forged so that they cancel, a permutation column that is not
    the one the constraints describe (constraint identity: reason 3)"""
    from p3_cases import EXT_W
    over = dict(queries=5, pow_bits=2)
    params(preset, **over)
    blob = hal.make_params(preset, **over)
    airs = p3.lookup_demo_airs(EXT_W[preset])
    tables, init = p3.lookup_demo_tables(5, 3, seed=2, airs=airs), p3.to_mont([6])
    pf = o.oracle_p3_prove(tables, init)
    assert o.oracle_p3_verify(tables, pf, init) == 0 == p3.verify(tables, pf, init, params=blob)

    def both(tabs):
        q = o.oracle_p3_prove(tabs, init)
        a, b = o.oracle_p3_verify(tabs, q, init), p3.verify(tabs, q, init, params=blob)
        assert a == b
        return a

    def with_cell(t, row, col, delta):
        tr = o.from_mont(tables[t].trace).astype(np.uint64)
        tr[row, col] = (int(tr[row, col]) + delta) % P
        return tables[:t] + [p3.Table.from_canonical(tables[t].air, tr)] + tables[t + 1:]

    assert both(with_cell(3, 2, 1, 1)) == 8          # the range table claims one more lookup than was made
    assert both(with_cell(1, 0, 3, P - 1)) == 8      # the add table one fewer
    cpu = o.from_mont(tables[0].trace)
    live = int(np.flatnonzero(cpu[:, 4] == 1)[0])
    assert both(with_cell(0, live, 2, 1)) == 8       # the cpu sends (a, b, a + b + 1): nobody receives that tuple
    # forged sums: +d on one table, -d on another keeps the total at zero, but phi[last] = cumsum fails (and every later challenge moves)
    at = 1 + len(tables) + 8 + 8                     # header | trace root | permutation root | the cumulative sums
    s = pf.copy()
    s[at] = (int(s[at]) + 5) % P
    s[at + 4] = (int(s[at + 4]) - 5) % P
    assert o.oracle_p3_verify(tables, s, init) == 3 == p3.verify(tables, s, init, params=blob)
    s = pf.copy()
    s[at] = (int(s[at]) + 5) % P
    assert o.oracle_p3_verify(tables, s, init) == 8 == p3.verify(tables, s, init, params=blob)
    # two defects at once: both verifiers report the same one (the stages of the check run in one order)
    summed = pf.copy()
    summed[at] = (int(summed[at]) + 5) % P
    forged = summed.copy()
    forged[at + 4] = (int(forged[at + 4]) - 5) % P
    for base, reason in ((summed, 8), (forged, 3)):
        for two in (base[:-3], np.concatenate([base, [0]]).astype(np.uint32)):      # ... and the last 3 words cut off / one trailing word
            assert o.oracle_p3_verify(tables, two, init) == reason == p3.verify(tables, two, init, params=blob)
    two = summed.copy()
    two[-1] = P                                      # ... and a word that is no field element
    assert o.oracle_p3_verify(tables, two, init) == 1 == p3.verify(tables, two, init, params=blob)
    high = [p3.Table(t.air, None, t.public_values) for t in tables]
    high[3].log_height = tables[3].log_height + 1    # ... and a pinned height the proof does not have
    assert o.oracle_p3_verify(high, summed, init) == 2 == p3.verify(high, summed, init, params=blob)
    for n in range(400):                             # every cut inside the header, the roots, the sums and the opened values
        assert o.oracle_p3_verify(tables, pf[:n], init) == p3.verify(tables, pf[:n], init, params=blob) != 0, n
    # the one known difference: the product checks the total length before any query, the oracle query by query -- a
    # changed last word (6 from both on its own) AND a trailing word (1 from both on its own) give 6 from the oracle
    two = np.concatenate([pf, [0]]).astype(np.uint32)
    two[pf.size - 1] = (int(two[pf.size - 1]) + 1) % P
    assert p3.verify(tables, two, init, params=blob) == 1
    # a verifier can pin a table's height (the range table must hold ALL values): the proof's own height word is not enough
    free = [p3.Table(t.air, None, t.public_values) for t in tables]
    assert p3.verify(free, pf, init, params=blob) == 0 == o.oracle_p3_verify(free, pf, init)       # heights from the proof
    pinned = [p3.Table(t.air, None, t.public_values) for t in tables]
    pinned[3].log_height = tables[3].log_height
    assert p3.verify(pinned, pf, init, params=blob) == 0 == o.oracle_p3_verify(pinned, pf, init)
    pinned[3].log_height = tables[3].log_height + 1
    assert p3.verify(pinned, pf, init, params=blob) == 2 == o.oracle_p3_verify(pinned, pf, init)
    # the same tables under an AIR whose lookup constraints were built for the other extension do not verify
    wrong = p3.lookup_demo_airs(EXT_W[1 - preset])
    wt = [p3.Table(a, t.trace, t.public_values) for a, t in zip(wrong, tables)]
    assert both(wt) == 3
    # random damage anywhere: the same verdict from both
    rng = np.random.default_rng(preset + 10)
    seen = set()
    for k in range(200):
        s = pf.copy()
        i = int(rng.integers(0, s.size))
        s[i] = (int(s[i]) + 1 + int(rng.integers(0, 9))) % P
        got, want = p3.verify(tables, s, init, params=blob), o.oracle_p3_verify(tables, s, init)
        assert got == want != 0, (k, i, got, want)
        seen.add(got)
    assert {5, 6} <= seen


@pytest.mark.parametrize("preset", [0, 1])
def test_hostile_proofs_are_rejected_by_both_verifiers_with_the_same_reason(params, preset):
    over = dict(queries=6, pow_bits=5)
    params(preset, **over)
    blob = hal.make_params(preset, **over)
    from p3_cases import air_of
    a1, a2 = air_of("cubic", 5), air_of("fib", None)
    t1 = p3.Table.from_canonical(a1, *p3.cubic_trace(5, 5, seed=3))
    t2 = p3.Table.from_canonical(a2, *p3.fibonacci_trace(3))
    tables, init = [t1, t2], p3.to_mont([4, 5])
    pf = o.oracle_p3_prove(tables, init)
    assert p3.verify(tables, pf, init, params=blob) == 0
    rng = np.random.default_rng(preset)
    seen = set()
    for k in range(500):
        s = pf.copy()
        kind = k % 6
        if kind == 0:
            i = int(rng.integers(0, s.size)); s[i] = (int(s[i]) + 1) % P
        elif kind == 1:
            i = int(rng.integers(0, s.size)); s[i] = int(rng.integers(P, 1 << 32))           # not a field element
        elif kind == 2:
            s = s[: int(rng.integers(0, s.size))]
        elif kind == 3:
            s = np.concatenate([s, rng.integers(0, P, size=int(rng.integers(1, 30)), dtype=np.uint32)])
        elif kind == 4:
            a, b = sorted(int(x) for x in rng.integers(0, s.size, size=2))
            s[a:b] = rng.integers(0, P, size=b - a, dtype=np.uint32)
        else:
            i = int(rng.integers(0, s.size)); s[i] ^= 1 << int(rng.integers(0, 30))
        got, want = p3.verify(tables, s, init, params=blob), o.oracle_p3_verify(tables, s, init)
        if np.array_equal(s, pf):
            continue
        assert got != 0 and want != 0
        assert got == want, (k, got, want)
        seen.add(got)
    assert {1, 5, 6} <= seen
    # a witness that breaks one constraint still yields a proof (Plonky3 checks constraints in debug builds only);
    # the constraint identity at zeta exposes it
    tr, pv = p3.cubic_trace(5, 5, seed=3)
    tr[7, 0] = (int(tr[7, 0]) + 1) % P
    bad = [p3.Table.from_canonical(a1, tr, pv), t2]
    assert a1.check_trace(tr, pv) != []
    pfb = o.oracle_p3_prove(bad, init)
    assert o.oracle_p3_verify(bad, pfb, init) == 3 and p3.verify(bad, pfb, init, params=blob) == 3


def test_quotient_degree_above_the_blowup_is_refused(params):
    params(1)           # blow-up 2: two chunks at most
    b = p3.AirBuilder(1)
    x = b.local(0)
    b.assert_zero(x * x * x * x - x)          # degree 4: four chunks
    air = b.build()
    t = p3.Table.from_canonical(air, np.zeros((4, 1), dtype=np.uint64))
    with pytest.raises(RuntimeError):
        o.oracle_p3_prove([t])
    assert p3.verify([t], np.zeros(100, dtype=np.uint32)) == -1


def test_full_parameter_set_verifier_threads_agree_with_the_oracle(params):
    """100 queries: rk_p3_verify checks them on several threads and reports the verdict of the FIRST failing query, the
    one a sequential verifier (the oracle's) gives"""
    case = "sp1_fib_k10_full"
    preset, over, _, _ = P3_CASES[case]
    params(preset, **over)
    blob = hal.make_params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf = o.oracle_p3_prove(tables, init)
    rng = np.random.default_rng(8)
    seen = set()
    for k in range(80):
        s = pf.copy()
        for _ in range(1 + k % 3):                      # one to three changed words: several queries may fail at once
            i = int(rng.integers(0, s.size))
            s[i] = (int(s[i]) + 1 + int(rng.integers(0, 5))) % P
        got, want = p3.verify(tables, s, init, params=blob), o.oracle_p3_verify(tables, s, init)
        assert got == want != 0, (k, got, want)
        seen.add(got)
    assert len(seen) >= 2
    assert p3.verify(tables, pf[:-3], init, params=blob) == 1 == o.oracle_p3_verify(tables, pf[:-3], init)


# ---------------------------------------------------------------- quotients in 4, 8 and 16 chunks
def _blowup(preset, over):
    return over.get("blowup_log2", hal.make_params(preset).blowup_log2)


def test_high_degree_cases_cover_every_stride_and_both_presets():
    """the seeded cases prove quotients of 4, 8 and 16 chunks under blow-ups 4, 8 and 16 in both parameter sets, at
    quotient-domain strides blowup_log2 - lqd of 0, 1, 3 and 4, lookups beside and inside a table of lqd >= 2; the
    exact reference runs on all of them but the 2^12-row table at qd = 16"""
    seen, strides, lookups = set(), set(), set()
    for case, (preset, over, _, _) in P3_CASES.items():
        blow = _blowup(preset, over)
        for k, lqd, perm in shapes(case):
            seen.add((preset, blow, lqd))
            strides.add(blow - lqd)
            if lqd >= 2 and perm:
                lookups.add((preset, blow - lqd))
    for preset in (0, 1):
        assert {(preset, 2, 2), (preset, 3, 2), (preset, 3, 3), (preset, 4, 3), (preset, 4, 4)} <= seen
    assert {0, 1, 3, 4} <= strides
    assert (0, 1) in lookups and (1, 1) in lookups
    assert shapes("sp1_blow4_deg17_k1") == [(1, 4, False)] and shapes("sp1_blow4_deg17_k12") == [(12, 4, False)]
    assert set(P3_CASES) - set(REF_CASES) == {"sp1_blow4_deg17_k12"}


@pytest.mark.parametrize("D,lqd", [(2, 0), (3, 1), (4, 2), (5, 2), (6, 3), (9, 3), (10, 4), (17, 4)])
def test_power_air_degree(D, lqd):
    from p3_cases import power_air, power_trace
    air = power_air(D)
    steps = np.ascontiguousarray(air.steps, dtype=np.uint32)
    assert air.log_quotient_degree() == lqd == air.info()["log_quotient_degree"]
    assert o.oracle().or_air_log_quotient_degree(o.OrAir(steps=steps.ctypes.data, n_steps=steps.shape[0])) == lqd
    tr, pv = power_trace(4, D, seed=D)
    assert air.check_trace(tr, pv) == []
    bad, pv2 = power_trace(4, D, seed=D, kick_row=6)
    assert not np.array_equal(bad, tr)
    assert air.check_trace(bad, pv2) == [(5, 3)]          # the degree-D transition into row 6, nothing else


@pytest.mark.parametrize("case", REF_CASES)
def test_exact_reference_matches_the_oracle_proof(params, case):
    """transcript, trace openings, quotient chunks and the zps recombination of tests/p3_ref.py against the oracle's
    proof words (lookup tables: their cumulative sums, permutation openings and quotients too)"""
    import p3_ref as R
    preset, over, _, _ = P3_CASES[case]
    R.p2_tables(preset)                    # read the preset's constants before the parameter set changes
    params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf = o.oracle_p3_prove(tables, init)
    R.check_proof(preset, _blowup(preset, over), tables, init, pf)


@pytest.mark.parametrize("preset", [0, 1])
@pytest.mark.parametrize("D", [5, 9, 17])
def test_broken_high_degree_trace_is_refused(params, preset, D):
    """lqd 2, 3, 4 at blow-up 16: a trace whose degree-D transition fails once is proven, and both verifiers refuse the
    proof with reason 3; the exact reference still reproduces the opened chunks, but their recombination is no longer
    fold(zeta) / Z_H(zeta)"""
    import p3_ref as R
    from p3_cases import air_of, power_trace
    R.p2_tables(preset)
    over = dict(queries=3, pow_bits=2, blowup_log2=4)
    params(preset, **over)
    blob = hal.make_params(preset, **over)
    air = air_of("power", D)
    good = [p3.Table.from_canonical(air, *power_trace(5, D, seed=70 + D))]
    bad = [p3.Table.from_canonical(air, *power_trace(5, D, seed=70 + D, kick_row=9))]
    init = p3.to_mont([D])
    pf = o.oracle_p3_prove(good, init)
    assert o.oracle_p3_verify(good, pf, init) == 0 == p3.verify(good, pf, init, params=blob)
    pfb = o.oracle_p3_prove(bad, init)
    assert o.oracle_p3_verify(bad, pfb, init) == 3 == p3.verify(bad, pfb, init, params=blob)
    with pytest.raises(AssertionError, match="zps recombination"):
        R.check_proof(preset, 4, bad, init, pfb)


def test_exact_reference_notices_a_changed_opening(params):
    """the reference is not vacuous: a chunk word or a trace word moved by one, or a root, is reported"""
    import p3_ref as R
    case = "sp1_blow4_lqd0_to_4"
    preset, over, _, _ = P3_CASES[case]
    R.p2_tables(preset)
    params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf = o.oracle_p3_prove(tables, init)
    head = 1 + len(tables) + 16
    at_chunks = head + sum(8 * t.air.width + (16 << t.air.log_quotient_degree()) for t in tables[:4]) + 8 * tables[4].air.width
    for at, what in ((head + 1, "table 0: trace_local"), (at_chunks + 16 * 11 + 5, "table 4: quotient chunk 11 of 16"),
                     (1 + len(tables) + 3, "trace_local")):
        s = pf.copy()
        s[at] = (int(s[at]) + 1) % P
        with pytest.raises(AssertionError, match=what):
            R.check_proof(preset, 4, tables, init, s)


# ---------------------------------------------------------------- the exact reference on tables with interactions
LOOKUP_REF_CASES = [c for c in REF_CASES if any(perm for _, _, perm in shapes(c))]


def test_lookup_cases_of_the_exact_reference():
    assert {"sp1_lookup_k6", "sp1_lookup_two_rows", "sp1_selfperm_k5", "risc0_lookup_k7_blow2", "sp1_merkle_paths_poseidon2_chip",
            "sp1_blow4_lookup_beside_deg9", "risc0_blow3_powerperm_deg5", "sp1_blow4_powerperm_deg9", "sp1_lookup_beside_plain",
            "sp1_wide_tuples_k9"} == set(LOOKUP_REF_CASES)


@pytest.mark.parametrize("case", LOOKUP_REF_CASES)
def test_exact_reference_checks_the_lookups_of_the_oracle_proof(params, case):
    """every table with interactions of every seeded case: the oracle's cumulative sums, permutation openings (all
    4 (nb + 1) base columns, at zeta and zeta g) and quotient chunks are the reference's; so are they in the O(n) mode
    for tall tables (barycentric openings, no dense quotient), which the GPU tests rely on above 2^11 rows"""
    import p3_ref as R
    preset, over, _, _ = P3_CASES[case]
    R.p2_tables(preset)
    params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf = o.oracle_p3_prove(tables, init)
    seen = {}
    R.check_proof(preset, _blowup(preset, over), tables, init, pf, perm_out=seen)
    assert sorted(seen) == [i for i, t in enumerate(tables) if t.air.perm_width] != []
    for ti, pt in seen.items():
        assert pt.shape == (1 << tables[ti].log_height, tables[ti].air.perm_width)
    assert R.check_proof(preset, _blowup(preset, over), tables, init, pf, tall=True) == R.check_proof(preset, _blowup(preset, over), tables, init, pf, quotient=False)


def test_eval_steps_covers_every_opcode():
    """no opcode of raiko_amd/p3.py is left to raise, and no table is skipped for having interactions"""
    import inspect
    import p3_ref as R
    src = inspect.getsource(R.eval_steps)
    for name in ("CONST", "LOCAL", "NEXT", "PUBLIC", "IS_FIRST_ROW", "IS_LAST_ROW", "IS_TRANSITION", "ADD", "SUB", "MUL", "NEG",
                 "ASSERT_ZERO", "PERM_LOCAL", "PERM_NEXT", "CHALLENGE", "CUMSUM"):
        assert "p3." + name in src, name
    assert max(p3.PERM_LOCAL, p3.PERM_NEXT, p3.CHALLENGE, p3.CUMSUM) == 15
    with pytest.raises(ValueError):
        R.eval_steps(p3.Air(np.array([[16, 0, 0]], dtype=np.uint32), 1, 0), np.zeros((1, 1, 4), dtype=np.uint64), np.zeros((1, 1, 4), dtype=np.uint64),
                     [], [np.zeros((1, 4), dtype=np.uint64)] * 3, (1, 0, 0, 0), 11)


@pytest.mark.parametrize("log_n,L,n_used,unbalanced", [(1, 3, 7, False), (4, 1, 1, False), (5, 2, 6, True), (6, 3, 7, True), (5, 16, 8, False),
                                                       (3, 3, 63, False), (3, 2, 64, False), (3, 3, 65, True), (3, 16, 120, False)])
def test_reference_permutation_trace_satisfies_the_definition(log_n, L, n_used, unbalanced):
    """tests/p3_ref.py::perm_trace against eval_permutation_constraints row by row, in plain integers, without any proof:
    per batch entry * prod rlc = sum +-mult * prod_(j != i) rlc_j; phi[0] = sum entries[0]; phi[r + 1] - phi[r] = sum
    entries[r + 1]; on the edge tables of tests/p3_lookup_cases.py (last batch of one, column and constant multiplicities
    0, 1, 2, p - 1, both kinds, tuples of 0 to 59 values, bus p - 1), whose own asserts hold"""
    import field_ref as F
    import p3_lookup_cases as LC
    import p3_ref as R
    W = 11
    t = LC.edge_table(log_n, L, n_used, seed=3, unbalanced=unbalanced)
    pch = ((5, 0, P - 1, 77), (P - 2, 1, 0, 12345))
    pt = R.perm_trace(t, pch, 1)
    LC.assert_edges(t, pt)
    its, n, nb = t.air.interactions, 1 << log_n, (L + 1) // 2
    assert pt.shape == (n, 4 * (nb + 1)) and pt.dtype == np.uint64 and int(pt.max()) < P
    tr = [[int(v) for v in row] for row in F.from_mont(t.trace)]
    beta_pow = [(1, 0, 0, 0)]
    for _ in range(max(len(it.value_cols) for it in its)):
        beta_pow.append(F.ext_mul(beta_pow[-1], pch[1], W))
    ext_row = lambda r, b: tuple(int(v) for v in pt[r, 4 * b:4 * b + 4])
    rows = range(n) if n <= 16 else sorted({0, 1, 2, n // 2 - 1, n // 2, n - 2, n - 1} | {int(v) for v in np.random.default_rng(log_n).integers(0, n, 6)})
    for r in rows:
        total = (0, 0, 0, 0)
        for b in range(nb):
            pair = its[2 * b:2 * b + 2]
            rlc, sm = [], []
            for it in pair:
                acc = F.ext_add(pch[0], (it.bus % P, 0, 0, 0))
                for j, c in enumerate(it.value_cols):
                    acc = F.ext_add(acc, F.ext_scale(beta_pow[j + 1], tr[r][c]))
                rlc.append(acc)
                m = it.mult if it.mult_is_const else tr[r][it.mult]
                sm.append(m % P if it.kind == p3.SEND else -m % P)
            lhs, rhs = ext_row(r, b), (0, 0, 0, 0)
            for i in range(len(pair)):
                lhs = F.ext_mul(lhs, rlc[i], W)
                term = (sm[i], 0, 0, 0)
                for j in range(len(pair)):
                    if j != i:
                        term = F.ext_mul(term, rlc[j], W)
                rhs = F.ext_add(rhs, term)
            assert lhs == rhs, (r, b)
            total = F.ext_add(total, ext_row(r, b))
        assert F.ext_sub(ext_row(r, nb), ext_row(r - 1, nb) if r else (0, 0, 0, 0)) == total, r


def test_edge_tables_are_proven_by_the_oracle_and_checked_by_the_reference(params):
    """the edge tables before they judge the GPU: the oracle proves them, both verifiers accept the balanced table and
    refuse its unbalanced twin with reason 8 (nonzero cumulative sum), and the exact reference reproduces cumulative sums,
    permutation openings and quotient chunks of both"""
    import p3_lookup_cases as LC
    import p3_ref as R
    R.p2_tables(1)
    over = dict(queries=3, pow_bits=1)
    params(1, **over)
    blob = hal.make_params(1, **over)
    init = p3.to_mont([4, 2])
    for log_n, L, n_used in ((1, 3, 7), (7, 3, 7), (5, 1, 1), (4, 2, 64), (6, 16, 8)):
        for unbalanced in (False, True):
            t = [LC.edge_table(log_n, L, n_used, seed=9, unbalanced=unbalanced)]
            pf = o.oracle_p3_prove(t, init)
            seen = {}
            R.check_proof(1, 1, t, init, pf, perm_out=seen)
            LC.assert_edges(t[0], seen[0])
            want = 8 if unbalanced else 0
            assert o.oracle_p3_verify(t, pf, init) == want == p3.verify(t, pf, init, params=blob), (log_n, L, n_used, unbalanced)


def test_exact_reference_notices_a_changed_lookup_word(params):
    """one word at a time in each class of words that only tables with interactions have: a cumulative sum, a perm_local
    word, a perm_next word, a chunk word of such a table -- each is reported under its own name"""
    import p3_ref as R
    case = "sp1_lookup_k6"
    preset, over, _, _ = P3_CASES[case]
    R.p2_tables(preset)
    params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf = o.oracle_p3_prove(tables, init)
    R.check_proof(preset, 1, tables, init, pf)
    nt = len(tables)
    cums = 1 + nt + 16
    head = cums + 4 * nt + 8                  # ... | the cumulative sums | quotient root | table 0: local, next, perm_local, perm_next, chunks
    t0, t1 = tables[0].air, tables[1].air
    pl0 = head + 8 * t0.width
    size0 = 8 * t0.width + 8 * t0.perm_width + (16 << t0.log_quotient_degree())
    pn1 = head + size0 + 8 * t1.width + 4 * t1.perm_width
    assert t0.perm_width == 12 and t1.perm_width == 8
    for at, what in ((cums + 4 * 2 + 1, "table 2: cumulative sum"), (cums, "table 0: cumulative sum"),
                     (pl0 + 4 * 9 + 2, "table 0: perm_local column 9 of 12"), (pl0, "table 0: perm_local column 0 of 12"),
                     (pn1 + 4 * 7 + 3, "table 1: perm_next column 7 of 8"),
                     (pl0 + 8 * t0.perm_width + 4 * 2 + 1, "table 0: quotient chunk 0 of 2"),
                     (pl0 + 8 * t0.perm_width + 16 + 4 * 3, "table 0: quotient chunk 1 of 2")):
        s = pf.copy()
        s[at] = (int(s[at]) + 1) % P
        with pytest.raises(AssertionError, match=what):
            R.check_proof(preset, 1, tables, init, s)


@pytest.mark.parametrize("k", [3, 8, 10])
def test_barycentric_opening_equals_the_dense_one(k):
    """tests/p3_ref.py::open_columns_at (O(n)) against interpolate + eval_base_poly_at (dense), both presets: columns of
    random values, a constant column, an impulse, all p - 1; at a random point and at that point times g"""
    import field_ref as F
    import p3_ref as R
    n = 1 << k
    for preset in (0, 1):
        W, gen = R.PRESETS[preset][:2]
        rng = np.random.default_rng(10 * k + preset)
        v = rng.integers(0, P, size=(n, 7), dtype=np.uint64)
        v[:, 3], v[:, 4], v[:, 5] = 5, 0, P - 1
        v[n - 1, 4] = 1
        C = R.interpolate(v, k, gen)
        z = tuple(int(c) for c in rng.integers(0, P, 4))
        for pt in (z, F.ext_scale(z, F.root(k, gen)), (int(z[0]), 0, 0, 0)):
            want = [tuple(int(c) for c in r) for r in R.eval_base_poly_at(C, pt, W)]
            assert R.open_columns_at(v, k, pt, preset) == want
            assert want[3] == (5, 0, 0, 0)
        a, b = R.openings(v, k, z, preset, tall=True), R.openings(v, k, z, preset)
        assert a == b


def test_more_than_120_used_columns_are_refused():
    """the staged tile holds 120 columns: 121 distinct columns read by the interactions are refused where the AIR is
    created, with the library's constraints or the front end's; 120 are taken"""
    import p3_lookup_cases as LC
    for L, n_used, fine in ((2, 120, True), (3, 121, False), (2, 122, False)):
        air, _ = LC.edge_air(L, n_used)
        own = air.steps[:int(np.flatnonzero(air.steps[:, 0] == p3.ASSERT_ZERO)[0]) + 1]        # the flag's constraint alone
        if fine:
            assert air.handle() is not None
            assert p3.Air(own, air.width, 0, air.interactions, append_lookup_constraints_w=11).n_constraints == air.n_constraints
            continue
        with pytest.raises(_lib.RkError) as ei:
            air.handle()
        assert ei.value.status == _lib.RK_ERR_INVALID
        with pytest.raises(_lib.RkError) as ei:
            p3.Air(own, air.width, 0, air.interactions, append_lookup_constraints_w=11)
        assert ei.value.status == _lib.RK_ERR_INVALID
