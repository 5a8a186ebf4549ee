"""The commit phase of the FRI query check as lookup tables (raiko_amd/fri_chip.py, rk_p3_fri_openings): the CPU side,
through the oracle as tests/test_p2_chip.py.  Honest shard proofs: the extracted public values and records agree with
the proof's own words, a transcript replay (tests/p3_ref.py) and a plain-Python replay of every fold chain over
tests/field_ref.py; the numpy witness satisfies all four AIRs; the oracle proves them and both verifiers accept.
Forged statements -- each kept self-consistent apart from the one thing named -- are proven by the oracle and refused
by both verifiers with the same reason."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import field_ref as FR
import fri_param_sets as PS
import oracle_lib as o
import p2_chip_ref as R
import p3_ref
from p3_cases import P3_CASES, init_of, tables_of
from raiko_amd import _lib, hal, p3
from raiko_amd import fri_chip as F

P = o.P
CASES = ["sp1_mixed_fib8_cubic4", "sp1_blow2_wide_k9"]     # two heights (a reduced opening joins mid-chain); blow-up 2


@pytest.fixture()
def params():
    yield o.oracle_set_params
    o.oracle_set_params()


def setup(params, case, **more):
    preset, over, _, _ = P3_CASES[case]
    over = dict(over, **more)
    params(preset, **over)
    blob = hal.make_params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    return blob, tables, init, o.oracle_p3_prove(tables, init)


def fri_part_of(tables, pf, blob):
    """the commit-phase part of a proof without lookups read straight from its words (layout: include/raiko_hip.h,
    rk_p3_prove) -> (canonical roots (R, 8), final 4, per query [(sibling 4, path (lfh, 8)) per round], position of n_rounds)"""
    nt = int(pf[0])
    assert not any(t.air.perm_width for t in tables)
    pos = 1 + nt + 8 + 8 + sum(8 * t.air.width + (16 << t.air.log_quotient_degree()) for t in tables)
    n_rounds = int(pf[pos])
    w = FR.from_mont(np.asarray(pf, dtype=np.uint64))
    roots = w[pos + 1: pos + 1 + 8 * n_rounds].reshape(n_rounds, 8)
    final = w[pos + 1 + 8 * n_rounds: pos + 5 + 8 * n_rounds]
    q0 = pos + 6 + 8 * n_rounds                                  # behind the proof-of-work witness
    log_max = max(int(v) for v in pf[1: 1 + nt]) + blob.blowup_log2
    assert n_rounds == log_max - blob.blowup_log2
    per_query = (pf.size - q0) // blob.queries
    assert q0 + per_query * blob.queries == pf.size
    tail = sum(4 + 8 * (log_max - 1 - rd) for rd in range(n_rounds))
    queries = []
    for qi in range(blob.queries):
        at = q0 + per_query * (qi + 1) - tail
        rounds = []
        for rd in range(n_rounds):
            lf = log_max - 1 - rd
            rounds.append((w[at: at + 4], w[at + 4: at + 4 + 8 * lf].reshape(lf, 8)))
            at += 4 + 8 * lf
        queries.append(rounds)
    return roots, final, queries, pos


def betas_of(preset, tables, init, pf, n_rounds, roots):
    """beta of every round from a replay of the transcript (tests/p3_ref.py's challenger; no lookups)"""
    head = p3_ref.parse(tables, pf)
    ch = p3_ref.Challenger(preset)
    ch.observe(FR.from_mont(init))
    ch.observe(head["trace_root"])
    for t in tables:
        ch.observe(FR.from_mont(t.public_values))
    ch.sample_ext()                                               # alpha
    ch.observe(head["quotient_root"])
    ch.sample_ext()                                               # zeta
    ch.sample_ext()                                               # the PCS's alpha
    out = []
    for rd in range(n_rounds):
        ch.observe(roots[rd])
        out.append(ch.sample_ext())
    return out


@pytest.mark.parametrize("case", CASES)
def test_honest_statement(params, case):
    blob, tables, init, pf = setup(params, case)
    rc, shape, pub, rec = F.fri_openings(tables, pf, init, blob)
    assert rc == 0 == p3.verify(tables, pf, init, params=blob)
    roots, final, queries, _ = fri_part_of(tables, pf, blob)
    L, Rn, Q = shape.log_max, shape.n_rounds, shape.queries
    assert (Rn, shape.blowup_log2, Q) == (roots.shape[0], blob.blowup_log2, blob.queries)
    assert case != CASES[0] or (Q, L, Rn) == (10, 9, 8)
    pubc = FR.from_mont(pub.astype(np.uint64))
    betas = betas_of(P3_CASES[case][0], tables, init, pf, Rn, roots)
    params(P3_CASES[case][0], **P3_CASES[case][1])                # the replay reads the preset's constants through the oracle: back to the case's set
    assert pubc.size == 12 * Rn + 4
    assert [tuple(int(v) for v in pubc[4 * r: 4 * r + 4]) for r in range(Rn)] == [tuple(b) for b in betas]
    assert np.array_equal(pubc[4 * Rn: 12 * Rn].reshape(Rn, 8), roots) and np.array_equal(pubc[12 * Rn:], final)
    # the records against the proof's words, and every fold chain replayed in plain Python over field_ref
    W, gen = int(blob.ext_w), int(blob.root_2_27)
    recc = FR.from_mont(rec.astype(np.uint64)).reshape(Q, -1)
    joined = 0
    for qi in range(Q):
        idx, at = int(recc[qi, 0]), 1
        assert idx < 1 << L
        folded = FR.ext([0, 0, 0, 0])
        for rd in range(Rn):
            lf = L - 1 - rd
            ro, sib, path = recc[qi, at: at + 4], recc[qi, at + 4: at + 8], recc[qi, at + 8: at + 8 + 8 * lf].reshape(lf, 8)
            at += 8 + 8 * lf
            assert np.array_equal(sib, queries[qi][rd][0]) and np.array_equal(path, queries[qi][rd][1])
            joined += bool(ro.any()) and rd > 0
            folded = FR.ext_add(folded, FR.ext(ro))
            e0, e1 = (FR.ext(sib), folded) if idx & 1 else (folded, FR.ext(sib))
            idx >>= 1
            x0 = pow(pow(gen, 1 << (27 - (lf + 1)), P), FR.bitrev(idx, lf), P)
            slope = FR.ext_scale(FR.ext_sub(e1, e0), FR.inv((-2 * x0) % P))
            folded = FR.ext_add(e0, FR.ext_mul(FR.ext_sub(FR.ext(betas[rd]), FR.ext([x0, 0, 0, 0])), slope, W))
        assert at == recc.shape[1]
        assert [int(v) for v in folded] == [int(v) for v in final]
    assert case != CASES[0] or joined == Q                      # the shorter table's reduced opening joins mid-chain
    st = F.Statement(shape, pub, rec, blob)
    rows = F.witness(st)
    assert [r.shape[0] for r in rows] == [1 << h for h in F.heights(shape)]
    pvs = [FR.from_mont(v.astype(np.uint64)) for v in F.public_values(st)]
    for air, r, pv in zip(F.airs(st), rows, pvs):
        assert air.log_quotient_degree() == 1
        assert air.check_trace(r, pv) == []
    chip = F.airs(st)[3]
    assert np.array_equal(rows[3], R.chip_trace(rows[3][:, :16], R.tables_of(), rows[3][:, -1]))   # the witness's Poseidon2 = the tests' restatement
    assert int(rows[3][:, -1].sum()) == Q * Rn + Q * F.steps_before(shape, Rn) and chip.width == 314
    assert all(int(t[:, m].sum()) == 0 for t, m in ((rows[0][Q * Rn:], F.FoldCols.REAL), (rows[2][Q * Rn:], 7)))   # padding: multiplicity 0
    tabs = F.tables_from_rows(st, rows)
    fp = o.oracle_p3_prove(tabs, st.init)
    assert o.oracle_p3_verify(tabs, fp, st.init) == 0 == p3.verify(tabs, fp, st.init, params=blob)
    assert F.verify_fri_statement(tables, pf, init, fp, blob) == 0


@pytest.mark.parametrize("pset,case", PS.ROW_IDS, ids=[PS.row_id(*x) for x in PS.ROW_IDS])
def test_reference_holds_under_parameter_sets(params, pset, case):
    """the oracle and the numpy witness alone under every set of tests/fri_param_sets.py; the witness's Poseidon2 against
    the tests' restatement under the oracle's tables and matrix"""
    st, rows = PS.check_reference(F, F.verify_fri_statement, pset, case)
    assert R.tables_of()[3] == int(st.params.p2_m4) and st.ext_w == int(st.params.ext_w)
    assert np.array_equal(rows[3], R.chip_trace(rows[3][:, :16], R.tables_of(), rows[3][:, -1]))
    assert [r.shape[0] for r in rows] == [1 << h for h in F.heights(st.shape)]


def test_mutated_shard_proofs_give_the_verifiers_verdict_and_no_records(params):
    blob, tables, init, pf = setup(params, CASES[0])
    seen = set()
    for k in (1, 3, pf.size // 3, pf.size // 2, pf.size - 40, pf.size - 3):
        bad = pf.copy()
        bad[k] = (int(bad[k]) + 1) % P
        rc, shape, pub, rec = F.fri_openings(tables, bad, init, blob)
        assert rc == p3.verify(tables, bad, init, params=blob) != 0 and shape is None and pub is None and rec is None
        seen.add(rc)
        with pytest.raises(_lib.RkError):
            F.statement(tables, bad, init, blob)
    assert len(seen) >= 2
    assert F.fri_openings(tables, pf[:-1], init, blob)[0] == 1
    assert np.array_equal(pf, o.oracle_p3_prove(tables, init)) and p3.verify(tables, pf, init, params=blob) == 0


class Forge:
    """the honest statement of CASES[0] and what a forger needs: canonical rows to vary, the verdict of both verifiers
    on the oracle's proof of a variation"""

    def __init__(self, params, pset=None):
        self.blob, self.tables, self.init, self.pf = setup(params, CASES[0]) if pset is None else PS.cpu_shard(pset, CASES[0])
        self.st = F.statement(self.tables, self.pf, self.init, self.blob)
        self.rows = F.witness(self.st)
        self.sh = self.st.shape
        self.fc, self.pc = F.FoldCols(self.sh), F.PathCols(self.sh)
        self.pub = FR.from_mont(self.st.publics.astype(np.uint64))
        self.tabs = R.tables_of()

    def copy(self):
        return [r.copy() for r in self.rows]

    def verdict(self, rows, pub=None):
        pub = self.pub if pub is None else pub
        Rn = self.sh.n_rounds
        pvs = [pub, pub[4 * Rn: 12 * Rn], [], []]
        tabs = [p3.Table.from_canonical(a, r, pv) for a, r, pv in zip(F.airs(self.st), rows, pvs)]
        q = o.oracle_p3_prove(tabs, self.st.init)
        a, b = o.oracle_p3_verify(tabs, q, self.st.init), p3.verify(tabs, q, self.st.init, params=self.blob)
        assert a == b
        return a

    def refold(self, rows, i, x0=None):
        """recompute e0 / e1 / folded of fold row i from its cur, sib, bit (and x0); the change of folded is taken out of
        the next row's joining reduced opening -- in the fold row and in the claims row -- so that the chain goes on unchanged"""
        fc, W = self.fc, int(self.blob.ext_w)
        row = rows[0][i]
        rd = int(row[fc.RD])
        cur, sib = FR.ext(row[fc.CUR: fc.CUR + 4]), FR.ext(row[fc.SIB: fc.SIB + 4])
        e0, e1 = (sib, cur) if row[fc.BIT] else (cur, sib)
        x0 = int(row[fc.X0]) if x0 is None else x0
        beta = FR.ext(self.pub[4 * rd: 4 * rd + 4])
        slope = FR.ext_scale(FR.ext_sub(e1, e0), FR.inv((-2 * x0) % P))
        new = FR.ext_add(e0, FR.ext_mul(FR.ext_sub(beta, FR.ext([x0, 0, 0, 0])), slope, W))
        delta = FR.ext_sub(new, FR.ext(row[fc.FOLDED: fc.FOLDED + 4]))
        row[fc.E0: fc.E0 + 4], row[fc.E1: fc.E1 + 4], row[fc.FOLDED: fc.FOLDED + 4], row[fc.X0] = e0, e1, new, x0
        self.shift_next_opening(rows, i, delta)

    def shift_next_opening(self, rows, i, delta):
        fc = self.fc
        nxt = rows[0][i + 1]
        assert nxt[fc.RD] == rows[0][i][fc.RD] + 1
        ro = FR.ext_sub(FR.ext(nxt[fc.RO: fc.RO + 4]), delta)
        nxt[fc.RO: fc.RO + 4] = ro
        rows[2][i + 1][3:7] = ro

    def path_at(self, q, rd):
        """(first path row, steps, first chip row) of query q's path in round rd"""
        lf = F.lfh(self.sh, rd)
        off = self.sh.queries * F.steps_before(self.sh, rd) + q * lf
        return off, lf, off + rd * self.sh.queries + q


@pytest.fixture()
def forge(params):
    return Forge(params)


def test_forged_fold_rows(forge):
    f, fc = forge, forge.fc
    Rn = f.sh.n_rounds
    assert f.verdict(f.rows) == 0
    rows = f.copy()                                   # a folded cell moved, the chain carried on: the fold equation
    i = 1 * Rn + 2
    rows[0][i][fc.FOLDED] = (int(rows[0][i][fc.FOLDED]) + 1) % P
    f.shift_next_opening(rows, i, FR.ext([1, 0, 0, 0]))
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # x0 negated in one round (its square, hence the next x0, stays): the domain point
    i = 2 * Rn + 3
    f.refold(rows, i, x0=(-int(rows[0][i][fc.X0])) % P)
    assert F.airs(f.st)[0].check_trace(rows[0], f.pub) != [] and f.verdict(rows) == 3
    rows = f.copy()                                   # a sibling value changed, pair and fold redone, the digest kept: no such leaf in the chip
    i = 3 * Rn + 4
    rows[0][i][fc.SIB + 1] = (int(rows[0][i][fc.SIB + 1]) + 1) % P
    f.refold(rows, i)
    assert F.airs(f.st)[0].check_trace(rows[0], f.pub) == [] and f.verdict(rows) == 8
    rows = f.copy()                                   # a claimed reduced opening changed: the claims table does not hold what the fold rows use
    rows[2][4 * Rn + 1][3] = (int(rows[2][4 * Rn + 1][3]) + 1) % P
    assert f.verdict(rows) == 8


def test_forged_public_values(forge):
    f = forge
    Rn = f.sh.n_rounds
    for at in (4 * 2 + 1, 4 * Rn + 8 * 3 + 5, 12 * Rn + 2):       # a beta word, a root word, a final-polynomial word
        pub = f.pub.copy()
        pub[at] = (int(pub[at]) + 1) % P
        assert f.verdict(f.rows, pub) == 3


@pytest.fixture(params=[None, "m4_0"], ids=["preset1", "m4_0"])
def forge_sets(request, params):
    return Forge(params, request.param)


def test_forged_path_bit_under_parameter_sets(forge_sets):
    """the first forgery of test_forged_paths once more under the other external matrix: still refused"""
    f, pc = forge_sets, forge_sets.pc
    off, lf, chip0 = f.path_at(3, 2)
    rows = f.copy()
    r = rows[1][off + lf - 1]
    r[pc.BIT] ^= 1
    left, right = r[pc.RIGHT: pc.RIGHT + 8].copy(), r[pc.LEFT: pc.LEFT + 8].copy()
    r[pc.LEFT: pc.LEFT + 8], r[pc.RIGHT: pc.RIGHT + 8] = left, right
    new = R.chip_trace(np.concatenate([left, right])[None, :], f.tabs)
    rows[3][chip0 + lf] = new[0]
    r[pc.PARENT: pc.PARENT + 8] = new[0, F.CHIP_OUT: F.CHIP_OUT + 8]
    assert f.tabs[3] == int(f.blob.p2_m4) and f.verdict(f.rows) == 0 and f.verdict(rows) == 3


def test_forged_paths(forge):
    f, pc = forge, forge.pc
    q, rd = 3, 2
    off, lf, chip0 = f.path_at(q, rd)
    assert lf >= 3
    rows = f.copy()                                   # the last step's bit flipped, left / right reordered to match, the compression redone:
    r = rows[1][off + lf - 1]                         # another position of the tree is opened (pos no longer follows the bits)
    r[pc.BIT] ^= 1
    left, right = r[pc.RIGHT: pc.RIGHT + 8].copy(), r[pc.LEFT: pc.LEFT + 8].copy()
    r[pc.LEFT: pc.LEFT + 8], r[pc.RIGHT: pc.RIGHT + 8] = left, right
    new = R.chip_trace(np.concatenate([left, right])[None, :], f.tabs)
    rows[3][chip0 + lf] = new[0]
    r[pc.PARENT: pc.PARENT + 8] = new[0, F.CHIP_OUT: F.CHIP_OUT + 8]
    pos_k = [k for row, k in F.airs(f.st)[1].check_trace(rows[1], f.pub[4 * f.sh.n_rounds: 12 * f.sh.n_rounds]) if row == off + lf - 1]
    assert len(pos_k) == 9                            # the eight root words and pos = bit on the last step
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # a path ended one step early (its last step and that compression dropped)
    rows[1][off + lf - 2][pc.LAST] = 1
    rows[1][off + lf - 1] = 0
    rows[3][chip0 + lf][-1] = 0
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # one query's path dropped: the fold row's opening is received by nobody
    rows[1][off: off + lf] = 0
    rows[3][chip0 + 1: chip0 + 1 + lf, -1] = 0
    assert F.airs(f.st)[1].check_trace(rows[1], f.pub[4 * f.sh.n_rounds: 12 * f.sh.n_rounds]) == [] and f.verdict(rows) == 8


def test_forged_padding_multiplicity(forge):
    """a padding row of the fold table made real, with everything it sends balanced -- the chip's zero-input padding row
    counted once, padding rows of the path and claims tables receiving -- so that the sums cancel: the AIRs refuse it"""
    f, fc, pc = forge, forge.fc, forge.pc
    n_real = f.sh.queries * f.sh.n_rounds
    rows = f.copy()
    assert not rows[0][n_real + 1].any() and not rows[3][-1][:16].any() and rows[3][-1][-1] == 0
    dig0 = rows[3][-1][F.CHIP_OUT: F.CHIP_OUT + 8]
    rows[0][n_real + 1][fc.REAL] = 1
    rows[0][n_real + 1][fc.DIG: fc.DIG + 8] = dig0
    rows[3][-1][-1] = 1
    rows[2][n_real + 1][7] = 1
    rows[1][-1][pc.CUR: pc.CUR + 8] = dig0
    rows[1][-1][pc.FIRST] = 1
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # left unbalanced, the lookups already refuse it
    rows[0][n_real + 1][fc.REAL] = 1
    assert f.verdict(rows) == 8


def test_verify_fri_statement(params):
    blob, tables, init, pf = setup(params, CASES[0])
    st = F.statement(tables, pf, init, blob)
    rows = F.witness(st)
    tabs = F.tables_from_rows(st, rows)
    fp = o.oracle_p3_prove(tabs, st.init)
    assert F.verify_fri_statement(tables, pf, init, fp, blob) == 0
    # a proof made for another shard proof: the same tables proven from other init words (other challenges, other openings)
    init2 = p3.to_mont([8, 6, 7])
    pf2 = o.oracle_p3_prove(tables, init2)
    st2 = F.statement(tables, pf2, init2, blob)
    fp2 = o.oracle_p3_prove(F.host_tables(st2), st2.init)
    assert F.verify_fri_statement(tables, pf2, init2, fp2, blob) == 0
    assert F.verify_fri_statement(tables, pf, init, fp2, blob) != 0 and F.verify_fri_statement(tables, pf2, init2, fp, blob) != 0
    # the same statement in tables of another height (the fold table padded to twice its rows): valid as a proof, refused by the pinned heights
    tall = [np.concatenate([rows[0], np.zeros_like(rows[0])])] + rows[1:]
    ttabs = F.tables_from_rows(st, tall)
    tp = o.oracle_p3_prove(ttabs, st.init)
    assert o.oracle_p3_verify(ttabs, tp, st.init) == 0 == p3.verify(ttabs, tp, st.init, params=blob)
    assert F.verify_fri_statement(tables, pf, init, tp, blob) == 2
    bad = pf.copy()                                   # a shard proof that is itself refused: its own reason
    bad[-3] = (int(bad[-3]) + 1) % P
    assert F.verify_fri_statement(tables, bad, init, fp, blob) == p3.verify(tables, bad, init, params=blob) != 0


def test_new_entry_points_refuse_malformed_arguments(params):
    blob, tables, init, pf = setup(params, CASES[0])
    lib = _lib.load()
    arr, keep = p3._c_tables(tables)
    n1, n2 = C.c_size_t(7), C.c_size_t(7)
    shape = np.zeros(4, dtype=np.uint32)
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    call = lambda par, sh, a, b: lib.rk_p3_fri_openings(par, arr, len(tables), u(init), init.size, u(pf), pf.size, sh, None, 0, None, 0, a, b)
    assert call(C.byref(blob), None, C.byref(n1), C.byref(n2)) == -1
    assert call(C.byref(blob), u(shape), None, C.byref(n2)) == -1 and call(C.byref(blob), u(shape), C.byref(n1), None) == -1
    assert lib.rk_p3_fri_openings(C.byref(blob), arr, len(tables), u(init), init.size, u(pf), pf.size, u(shape), None, 5, None, 0, C.byref(n1), C.byref(n2)) == -1
    assert lib.rk_p3_fri_openings(C.byref(blob), None, 0, None, 0, None, 0, u(shape), None, 0, None, 0, C.byref(n1), C.byref(n2)) == -1
    # too small: RK_ERR_CAPACITY with the sizes needed, nothing written
    assert call(C.byref(blob), u(shape), C.byref(n1), C.byref(n2)) == _lib.RK_ERR_CAPACITY and not shape.any()
    sh = F.Shape(9, 8, 1, 10)
    assert (n1.value, n2.value) == (12 * 8 + 4, 10 * F.per_record(sh))
    # the width-24 parameter set and a fold by 16 are outside the scope
    wide = hal.make_params(0, queries=10)
    assert call(C.byref(wide), u(shape), C.byref(n1), C.byref(n2)) == -1
    by16 = hal.make_params(1, queries=10, pow_bits=7, fri_fold_log2=4)
    assert call(C.byref(by16), u(shape), C.byref(n1), C.byref(n2)) == -1
    with pytest.raises(_lib.RkError):
        F.statement(tables, pf, init, wide)
    with pytest.raises(_lib.RkError):
        F.verify_fri_statement(tables, pf, init, pf, wide)
    del keep
    out = _lib.RkFriChipSizeInfo()
    assert lib.rk_fri_chip_sizes(9, 1, 10, None) == -1
    for lm, bl, q in ((9, 0, 10), (9, 5, 10), (2, 2, 10), (25, 1, 10), (9, 1, 0), (9, 1, 257)):
        assert lib.rk_fri_chip_sizes(lm, bl, q, C.byref(out)) == -1
    assert lib.rk_fri_chip_sizes(9, 1, 10, C.byref(out)) == 0
    sz = F.sizes(sh)
    assert (sz["fold_rows"], sz["path_rows"], sz["chip_rows"]) == (80, 360, 440)
    assert (sz["fold_width"], sz["path_width"], sz["claims_width"], sz["chip_width"]) == (F.FoldCols(sh).width, F.PathCols(sh).width, F.CLAIMS_WIDTH, 314)
    assert (sz["fold_log_height"], sz["path_log_height"], sz["claims_log_height"], sz["chip_log_height"]) == F.heights(sh)
    assert (sz["publics_words"], sz["records_words"]) == (100, 10 * F.per_record(sh))
    big = F.sizes(F.Shape(21, 20, 1, 100))                            # SP1's full set over a 2^20-row shard
    assert (big["fold_rows"], big["path_rows"], big["chip_rows"]) == (2000, 21000, 23000)
    assert lib.rk_fri_chip_rows_device(None, 9, 1, 10, None, None, None, 0, None, 0, None, 0, None, 0) == -1


def test_kernel_lanes_on_the_cpu(params, tmp_path):
    """the lane bodies of rk_fri_chip_rows_device (p3_kernels.hpp), run one emulated lane at a time in launch order
    (tests/emul/emul_fri.cpp), write the numpy witness word for word"""
    so = str(tmp_path / "libemul_fri.so")
    src = os.path.join(o.EMUL_DIR, "emul_fri.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(o.ROOT, "raiko_amd", "csrc"), "-o", so, src],
                   check=True, capture_output=True)
    lib = C.CDLL(so)
    for pset, case in [(None, c) for c in CASES] + PS.ROW_IDS:       # the sets: fri_path_lane<0>, other tables, another field
        blob, tables, init, pf = setup(params, case) if pset is None else PS.cpu_shard(pset, case)
        st = F.statement(tables, pf, init, blob)
        want = [p3.to_mont(r) for r in F.witness(st)]
        rc_ext, rc_int, diag, m4 = R.tables_of()
        tab = p3.to_mont(np.concatenate([rc_ext.reshape(-1), rc_int, diag]))
        got = [np.zeros_like(w) for w in want]
        sh = st.shape
        gen_l = int(p3.to_mont([pow(sh.root_2_27, 1 << (27 - sh.log_max), P)])[0])
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        lib.emul_fri_chip_rows(sh.log_max, sh.blowup_log2, sh.queries, gen_l, int(p3.to_mont([st.ext_w])[0]), vp(st.publics), vp(st.records),
                               vp(tab), m4, *[vp(g) for g in got], C.c_size_t(got[3].shape[0]))
        assert m4 == int(blob.p2_m4)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (pset, case)
