"""The reduced openings of the FRI query check as a lookup table (raiko_amd/fri_reduce.py, rk_p3_fri_inputs): the CPU side,
through the oracle as tests/test_fri_chip.py.  Honest shard proofs: layout, public values and records agree with the
proof's own words, and a plain-Python replay of the GROUPED form -- (sum alpha^k p_k(x) - S) / (x - z) per matrix and
point, big integers, X from the index -- gives for every (query, round) the joining reduced opening that
rk_p3_fri_openings reports from the verifier's term-by-term loop; the numpy witness satisfies all four AIRs; the oracle
proves them and both verifiers accept.  Forged statements -- each kept self-consistent apart from the one thing named --
are proven by the oracle and refused by both verifiers with the same reason."""
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
import threshold_cases as T
from p3_cases import P3_CASES, init_of, tables_of
from raiko_amd import _lib, hal, p3
from raiko_amd import fri_chip as F
from raiko_amd import fri_reduce as G

P = o.P
# two heights and public values; three tables on one alpha-power chain; a permutation batch shorter than the trace batch;
# blow-up 2
CASES = ["sp1_mixed_fib8_cubic4", "sp1_same_height", "sp1_lookup_beside_plain", "sp1_blow2_wide_k9"]


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


def opened_rows_of(tables, pf, shape, layout):
    """per query trows | prows | qrows read straight from the proof's words (layout: include/raiko_hip.h, rk_p3_prove)"""
    L, Rn, Q = shape.log_max, shape.n_rounds, shape.queries
    trow = sum(m.width for m in layout if m.batch == 0)
    prow = sum(m.width for m in layout if m.batch == 1)
    qrow = sum(m.width for m in layout if m.batch == 2)
    log_pmax = max([m.log_n + shape.blowup_log2 for m in layout if m.batch == 1], default=0)
    tail = sum(4 + 8 * (L - 1 - rd) for rd in range(Rn))
    per_query = trow + 8 * L + (prow + 8 * log_pmax if prow else 0) + qrow + 8 * L + tail
    q0 = pf.size - Q * per_query
    out = []
    for qi in range(Q):
        at = q0 + qi * per_query
        t = pf[at: at + trow]
        at += trow + 8 * L
        p_ = pf[at: at + prow]
        at += (prow + 8 * log_pmax) if prow else 0
        out.append(np.concatenate([t, p_, pf[at: at + qrow]]))
    return np.stack(out)


def ext_pow_chain(alpha, n, W):
    out, cur = [], [1, 0, 0, 0]
    for _ in range(n):
        out.append(cur)
        cur = F._ext_mul(cur, alpha, W)
    return out


@pytest.mark.parametrize("case", CASES)
def test_capture(params, case):
    blob, tables, init, pf = setup(params, case)
    rc, shape, layout, pub, rec = G.fri_inputs(tables, pf, init, blob)
    assert rc == 0 == p3.verify(tables, pf, init, params=blob)
    rc2, shape2, fpub, frec = F.fri_openings(tables, pf, init, blob)
    assert rc2 == 0 and shape2 == shape
    L, Rn, Q, W = shape.log_max, shape.n_rounds, shape.queries, int(blob.ext_w)
    # the layout from widths and proof header
    nt = int(pf[0])
    log_n = [int(v) for v in pf[1: 1 + nt]]
    want = G.layout_of(shape, [t.air.width for t in tables], [t.air.perm_width for t in tables], log_n,
                       [t.air.log_quotient_degree() for t in tables])
    assert layout == want and max(log_n) + shape.blowup_log2 == L
    if case == "sp1_lookup_beside_plain":
        assert 0 < sum(m.batch == 1 for m in layout) < sum(m.batch == 0 for m in layout)
    if case == "sp1_same_height":
        assert len({m.rd for m in layout}) == 1
    # the records: the index rk_p3_fri_openings reports, the rows the proof holds
    per = 1 + sum(m.width for m in layout)
    recs = rec.reshape(Q, per)
    assert np.array_equal(recs[:, 0], frec.reshape(Q, -1)[:, 0])
    assert np.array_equal(recs[:, 1:], opened_rows_of(tables, pf, shape, layout))
    # the public values: zeta from a replay of the transcript, A and S from the opened values at the absolute powers
    head = p3_ref.parse(tables, pf)
    pubc = [int(v) for v in FR.from_mont(pub.astype(np.uint64))]
    alpha, zeta = pubc[0:4], pubc[4:8]
    assert tuple(zeta) == tuple(int(v) for v in p3_ref.transcript(P3_CASES[case][0], tables, FR.from_mont(init), head)[1])
    params(P3_CASES[case][0], **P3_CASES[case][1])
    assert any(zeta[1:])
    ys = []
    batches = {0: ("local", "next"), 1: ("perm_local", "perm_next")}
    perm_tables = [i for i, t in enumerate(tables) if t.air.perm_width]
    chunk_at = [(i, j) for i, t in enumerate(tables) for j in range(1 << t.air.log_quotient_degree())]
    for b in (0, 1, 2):
        for k, m in enumerate([m for m in layout if m.batch == b]):
            if b == 2:
                i, j = chunk_at[k]
                ys.append([head["tables"][i]["chunks"][j]])
            else:
                i = k if b == 0 else perm_tables[k]
                ys.append([head["tables"][i][name] for name in batches[b]])
    used = {}
    at = 8
    groups = []                                        # per matrix: [(A, S, z)] per point
    for m, y in zip(layout, ys):
        gs = []
        for j in range(m.points):
            off = used.get(m.rd, 0)
            pw = ext_pow_chain(alpha, off + m.width, W)[off:]
            used[m.rd] = off + m.width
            S = [0, 0, 0, 0]
            for c in range(m.width):
                S = [(a + b) % P for a, b in zip(S, F._ext_mul(pw[c], list(y[j][c]), W))]
            assert pubc[at: at + 4] == pw[0] and pubc[at + 4: at + 8] == S
            g = pow(int(blob.root_2_27), 1 << (27 - m.log_n), P) if j else 1
            gs.append((pw[0], S, [v * g % P for v in zeta]))
            at += 8
        groups.append(gs)
    assert at == len(pubc)
    # the grouped replay against the verifier's term-by-term reduced openings
    frecs = FR.from_mont(frec.astype(np.uint64)).reshape(Q, -1)
    rows = FR.from_mont(recs[:, 1:].astype(np.uint64))
    offs = np.concatenate([[0], np.cumsum([m.width for m in layout])])
    sh_ = int(blob.coset_shift)
    for qi in range(Q):
        idx = int(FR.from_mont(recs[qi, :1].astype(np.uint64))[0])
        for rd in range(Rn):
            lh = L - rd
            x = sh_ * pow(pow(int(blob.root_2_27), 1 << (27 - lh), P), FR.bitrev(idx >> rd, lh), P) % P
            rop = [0, 0, 0, 0]
            for i, m in enumerate(layout):
                if m.rd != rd:
                    continue
                for A, S, z in groups[i]:
                    acc, pw = [0, 0, 0, 0], A
                    for c in range(m.width):
                        acc = [(a + b * int(rows[qi, offs[i] + c])) % P for a, b in zip(acc, pw)]
                        pw = F._ext_mul(pw, alpha, W)
                    den = [(x - z[0]) % P] + [-v % P for v in z[1:]]
                    quot = F._ext_mul([(a - b) % P for a, b in zip(acc, S)], G.ext_inv(den, W), W)
                    rop = [(a + b) % P for a, b in zip(rop, quot)]
            at_r = F.rec_round(shape, rd)
            assert rop == [int(v) for v in frecs[qi, at_r: at_r + 4]], (qi, rd)
    # the reduce table's row count
    st = G.Statement(F.Statement(shape, fpub, frec, blob), layout, pub, rec, blob)
    empty = Rn - len({m.rd for m in layout})
    assert G.sizes(st)["reduce_rows"] == Q * (sum(m.width for m in layout) + empty) == Q * G.rows_per_query(st.slots)
    assert sum(s.matrix is None for s in st.slots) == empty


def test_ext_inv():
    rng = np.random.default_rng(5)
    for _ in range(20):
        a = [int(v) for v in rng.integers(0, P, size=4)]
        assert F._ext_mul(a, G.ext_inv(a, 11), 11) == [1, 0, 0, 0]


def test_mutated_shard_proofs_give_the_verifiers_verdict_and_no_records(params):
    blob, tables, init, pf = setup(params, CASES[0])
    seen = set()
    for k in (1, 3, pf.size // 3, pf.size // 2, pf.size - 40, pf.size - 3):
        bad = pf.copy()
        bad[k] = (int(bad[k]) + 1) % P
        out = G.fri_inputs(tables, bad, init, blob)
        assert out[0] == p3.verify(tables, bad, init, params=blob) != 0 and out[1:] == (None, None, None, None)
        seen.add(out[0])
        with pytest.raises(_lib.RkError):
            G.statement(tables, bad, init, blob)
    assert len(seen) >= 2
    assert G.fri_inputs(tables, pf[:-1], init, blob)[0] == 1


def test_new_entry_points_refuse_malformed_arguments(params):
    blob, tables, init, pf = setup(params, CASES[0])
    lib = _lib.load()
    arr, keep = p3._c_tables(tables)
    n = [C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)]
    shape = np.zeros(4, dtype=np.uint32)
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    nn = [C.byref(v) for v in n]
    call = lambda par, sh, a, b, c: lib.rk_p3_fri_inputs(par, arr, len(tables), u(init), init.size, u(pf), pf.size, sh, None, 0, None, 0, None, 0, a, b, c)
    assert call(C.byref(blob), None, *nn) == -1
    for k in range(3):
        assert call(C.byref(blob), u(shape), *[None if j == k else nn[j] for j in range(3)]) == -1
    assert lib.rk_p3_fri_inputs(C.byref(blob), arr, len(tables), u(init), init.size, u(pf), pf.size, u(shape), None, 5, None, 0, None, 0, *nn) == -1
    assert lib.rk_p3_fri_inputs(C.byref(blob), None, 0, None, 0, None, 0, u(shape), None, 0, None, 0, None, 0, *nn) == -1
    # too small: RK_ERR_CAPACITY with the sizes needed, nothing written
    assert call(C.byref(blob), u(shape), *nn) == _lib.RK_ERR_CAPACITY and not shape.any()
    assert [v.value for v in n] == [5 * 5, 8 + 8 * 7, 10 * (1 + 2 + 5 + 12)]
    wide = hal.make_params(0, queries=10)              # the width-24 parameter set and a fold by 16 are outside the scope
    assert call(C.byref(wide), u(shape), *nn) == -1
    by16 = hal.make_params(1, queries=10, pow_bits=7, fri_fold_log2=4)
    assert call(C.byref(by16), u(shape), *nn) == -1
    with pytest.raises(_lib.RkError):
        G.statement(tables, pf, init, wide)
    with pytest.raises(_lib.RkError):
        G.verify_reduce_statement(tables, pf, init, pf, wide)
    del keep
    st = G.statement(tables, pf, init, blob)
    lw = st.layout_words
    out = _lib.RkFriReduceSizeInfo()
    sizes = lambda lm, bl, q, words, nm: lib.rk_fri_reduce_sizes(lm, bl, q, u(words) if words is not None else None, nm, C.byref(out))
    assert lib.rk_fri_reduce_sizes(9, 1, 10, u(lw), 5, None) == -1
    assert sizes(9, 1, 10, None, 5) == -1 and sizes(9, 1, 10, lw, 0) == -1
    for lm, bl, q in ((9, 0, 10), (9, 5, 10), (2, 2, 10), (25, 1, 10), (9, 1, 0), (9, 1, 257), (10, 1, 10), (9, 2, 10)):
        assert sizes(lm, bl, q, lw, 5) == -1          # the last two: a layout that does not fit the shape
    for at, v in ((0, 3), (1, 8), (2, 0), (3, 1), (4, 7), (10, 0)):   # batch, round, width, points, log_n; batches out of order
        bad = np.array(st.layout, dtype=np.uint64).reshape(-1)
        bad[at] = v
        assert sizes(9, 1, 10, p3.to_mont(bad), 5) == -1
    assert sizes(9, 1, 10, lw, 5) == 0
    sz = G.sizes(st)
    assert (sz["n_slots"], sz["rows_per_query"], sz["reduce_rows"]) == (len(st.slots), 25, 250)
    assert (sz["fold_width"], sz["path_width"], sz["reduce_width"], sz["chip_width"]) == (F.FoldCols(st.shape).width + 1, F.PathCols(st.shape).width, 38 + 11, 314)
    assert (sz["fold_log_height"], sz["path_log_height"], sz["reduce_log_height"], sz["chip_log_height"]) == G.heights(st)
    assert (sz["fold_publics_words"], sz["fold_records_words"], sz["reduce_publics_words"], sz["inputs_words"]) == \
        (st.fold.publics.size, st.fold.records.size, st.reduce_publics.size, st.in_records.size)
    assert lib.rk_fri_reduce_rows_device(None, 9, 1, 10, u(lw), 5, None, None, None, None, None, 0, None, 0, None, 0, None, 0) == -1


def test_default_fold_air_is_unchanged(params):
    """the new argument of fri_fold_air: without it the AIR is step for step the one of the parent statement; with it one
    column, one constraint and one claim value more"""
    sh = F.Shape(9, 8, 1, 10)
    a, b = F.fri_fold_air(sh), F.fri_fold_air(sh, coset_shift=31)
    assert a.width + 1 == b.width and len(a.interactions[2].value_cols) + 1 == len(b.interactions[2].value_cols)
    assert b.interactions[2].value_cols[3] == a.width
    assert a.log_quotient_degree() == b.log_quotient_degree() == 1


@pytest.mark.parametrize("case", CASES)
def test_honest_statement(params, case):
    blob, tables, init, pf = setup(params, case)
    st = G.statement(tables, pf, init, blob)
    rows = G.witness(st)
    assert [r.shape[0] for r in rows] == [1 << h for h in G.heights(st)]
    pvs = [FR.from_mont(v.astype(np.uint64)) for v in G.public_values(st)]
    for air, r, pv in zip(G.airs(st), rows, pvs):
        assert air.log_quotient_degree() == 1 and air.width == r.shape[1]
        assert air.check_trace(r, pv) == []
    c = G.ReduceCols(len(st.slots))
    n_real = st.shape.queries * G.rows_per_query(st.slots)
    assert int(rows[2][:, c.RCV].sum()) == st.shape.queries * st.shape.n_rounds and not rows[2][n_real:].any()
    tabs = G.tables_from_rows(st, rows)
    fp = o.oracle_p3_prove(tabs, st.init)
    assert o.oracle_p3_verify(tabs, fp, st.init) == 0 == p3.verify(tabs, fp, st.init, params=blob)
    assert G.verify_reduce_statement(tables, pf, init, fp, blob) == 0


@pytest.mark.parametrize("pset,case", PS.ROW_IDS, ids=[PS.row_id(*x) for x in PS.ROW_IDS])
def test_reference_holds_under_parameter_sets(params, pset, case):
    """the oracle and the numpy witness alone under every set of tests/fri_param_sets.py"""
    st, rows = PS.check_reference(G, G.verify_reduce_statement, pset, case)
    assert (st.ext_w, st.coset_shift) == (int(st.params.ext_w), int(st.params.coset_shift))
    assert [r.shape[0] for r in rows] == [1 << h for h in G.heights(st)]
    c = G.ReduceCols(len(st.slots))
    assert int(rows[2][:, c.RCV].sum()) == st.shape.queries * st.shape.n_rounds


class Forge:
    """the honest statement of CASES[0] and what a forger needs: canonical rows to vary, the verdict of both verifiers on
    the oracle's proof of a variation"""

    def __init__(self, params, pset=None):
        self.blob, self.tables, self.init, self.pf = setup(params, CASES[0]) if pset is None else PS.cpu_shard(pset, CASES[0])
        self.st = G.statement(self.tables, self.pf, self.init, self.blob)
        self.rows = G.witness(self.st)
        self.sh, self.slots = self.st.shape, self.st.slots
        self.c = G.ReduceCols(len(self.slots))
        self.fx = F.FoldCols(self.sh).width                   # the X column of fold'
        self.pubs = [FR.from_mont(v.astype(np.uint64)) for v in G.public_values(self.st)]
        self.rec = p3.from_mont(self.st.in_records).astype(np.uint64).reshape(self.sh.queries, self.st.per_record)
        self.rpq = G.rows_per_query(self.slots)
        self.air = G.airs(self.st)[2]

    def copy(self):
        return [r.copy() for r in self.rows]

    def at(self, q, m, col=0):
        return q * self.rpq + self.slots[m].row0 + col

    def bad_rows(self, rows, pub=None):
        return sorted({r for r, _ in self.air.check_trace(rows[2], self.pubs[2] if pub is None else pub)})

    def verdict(self, rows, pubs=None):
        pubs = self.pubs if pubs is None else pubs
        tabs = [p3.Table.from_canonical(a, r, pv) for a, r, pv in zip(G.airs(self.st), rows, pubs)]
        q = o.oracle_p3_prove(tabs, self.st.init)
        a, b = o.oracle_p3_verify(tabs, q, self.st.init), p3.verify(tabs, q, self.st.init, params=self.blob)
        assert a == b
        return a


@pytest.fixture()
def forge(params):
    return Forge(params)


def bump(row, col, by=1):
    row[col] = (int(row[col]) + by) % P


def test_forged_opened_values(forge):
    f, c = forge, forge.c
    assert f.verdict(f.rows) == 0
    q, m, col = 3, 1, 2                               # query 3, the quotient chunk of the tall table, its third column
    assert f.slots[m].points == 1 and f.slots[0].points == 2
    rows = f.copy()                                   # a changed P and nothing else: the running sums no longer follow
    bump(rows[2][f.at(q, m, col)], c.PV)
    assert f.bad_rows(rows) == [f.at(q, m, col) - 1] and f.verdict(rows) == 3
    rows = f.copy()                                   # a changed P, the table redone from it: valid in itself, but the round's
    rec = f.rec.copy()                                # reduced opening is not the one the fold chain uses
    bump(rec[q], 1 + f.slots[m].rec_off + col)
    rows[2] = G.reduce_rows(f.st, records=rec)
    assert f.bad_rows(rows) == [] and f.verdict(rows) == 8
    # ONE cell for both points: a P with which only the sum at zeta gen is redone (the sum at zeta kept as for the
    # honest value) breaks the sum at zeta, and the other way round -- both constraints read the same cell
    q, m, col = 2, 0, 1
    rec = f.rec.copy()
    bump(rec[q], 1 + f.slots[m].rec_off + col)
    redone = G.reduce_rows(f.st, records=rec)
    r = f.at(q, m, col)
    for keep, other in ((0, 1), (1, 0)):
        rows = f.copy()
        rows[2][r] = redone[r]
        for at in (c.SUM[keep], c.QUOT[keep]):
            rows[2][r][at: at + 4] = f.rows[2][r][at: at + 4]
        quot = [(int(a) + int(b)) % P for a, b in zip(rows[2][r][c.QUOT[0]: c.QUOT[0] + 4], rows[2][r][c.QUOT[1]: c.QUOT[1] + 4])]
        rows[2][r][c.ROP: c.ROP + 4] = quot           # the first matrix of its round: ROP = the two quotients
        bad = {k for row, k in f.air.check_trace(rows[2], f.pubs[2]) if row == r - 1}
        assert bad                                     # the transition into the row: the kept sum does not follow from P
        rows[2][r][c.PV] = f.rows[2][r][c.PV]          # the honest P back: now the redone sum is the one that does not follow
        bad2 = {k for row, k in f.air.check_trace(rows[2], f.pubs[2]) if row == r - 1}
        assert bad2 and bad2.isdisjoint(bad)
        rows[2][r][c.PV] = redone[r][c.PV]
        assert f.verdict(rows) == 3


def test_forged_opened_value_under_the_other_matrix(params):
    """the first two forgeries of test_forged_opened_values once more under m4_0: still refused, for the same reasons"""
    f = Forge(params, "m4_0")
    c = f.c
    assert int(f.blob.p2_m4) == 0 and f.verdict(f.rows) == 0
    q, m, col = 3, 1, 2
    rows = f.copy()
    bump(rows[2][f.at(q, m, col)], c.PV)
    assert f.bad_rows(rows) == [f.at(q, m, col) - 1] and f.verdict(rows) == 3
    rows = f.copy()
    rec = f.rec.copy()
    bump(rec[q], 1 + f.slots[m].rec_off + col)
    rows[2] = G.reduce_rows(f.st, records=rec)
    assert f.bad_rows(rows) == [] and f.verdict(rows) == 8


def test_forged_running_cells(forge):
    f, c = forge, forge.c
    q, m = 4, 5                                       # the short table's trace matrix (two points, width 5)
    assert f.slots[m].points == 2 and f.slots[m].width == 5
    for col, at in ((4, c.QUOT[0] + 1), (4, c.QUOT[1]), (2, c.POW[0] + 2), (3, c.POW[1]), (1, c.SUM[0]), (2, c.SUM[1] + 3)):
        rows = f.copy()
        bump(rows[2][f.at(q, m, col)], at)
        assert f.bad_rows(rows) != [] and f.verdict(rows) == 3
    rows = f.copy()                                   # a quotient and the running reduced opening moved together: the division
    r = rows[2][f.at(q, m, 4)]
    bump(r, c.QUOT[0])
    bump(r, c.ROP)
    assert f.bad_rows(rows) == [f.at(q, m, 4)] and f.verdict(rows) == 3


def test_forged_schedule(forge):
    f, c = forge, forge.c
    n_real = f.sh.queries * f.rpq
    q, m = 5, 5
    rows = f.copy()                                   # a column row dropped (the rows behind it move up)
    rows[2] = np.concatenate([np.delete(rows[2], f.at(q, m, 2), axis=0), np.zeros((1, c.width), dtype=np.uint64)])
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # a column row twice (the last padding row falls off)
    rows[2] = np.insert(rows[2], f.at(q, m, 2), rows[2][f.at(q, m, 2)], axis=0)[:-1]
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # a whole matrix dropped from one query
    lo, hi = f.at(q, m), f.at(q, m) + f.slots[m].width
    rows[2] = np.concatenate([np.delete(rows[2], np.s_[lo:hi], axis=0), np.zeros((hi - lo, c.width), dtype=np.uint64)])
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # two matrices of one round swapped (each row keeps its own cells)
    a0, a1, w0, w1 = f.at(q, 0), f.at(q, 1), f.slots[0].width, f.slots[1].width
    assert f.slots[0].rd == f.slots[1].rd and a1 == a0 + w0
    blk = np.concatenate([f.rows[2][a1: a1 + w1], f.rows[2][a0: a0 + w0]])
    rows[2][a0: a0 + w0 + w1] = blk
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # a real row behind the last query: the table must end with a whole query
    rows[2][n_real] = rows[2][0]
    rows[2][n_real][c.Q] = f.sh.queries
    assert f.verdict(rows) == 3


def test_forged_empty_round_and_padding(forge):
    f, c, pc = forge, forge.c, F.PathCols(forge.sh)
    m = next(i for i, s in enumerate(f.slots) if s.matrix is None)
    q = 6
    rows = f.copy()                                   # a nonzero reduced opening on a round without a matrix, with a quotient
    r = rows[2][f.at(q, m)]                           # that explains it and the fold row using it (the claim is received)
    bump(r, c.ROP)
    bump(r, c.QUOT[0])
    bump(rows[0][q * f.sh.n_rounds + f.slots[m].rd], F.FoldCols.RO)
    assert f.bad_rows(rows) == [f.at(q, m)] and f.verdict(rows) == 3
    n_real = f.sh.queries * f.rpq
    rows = f.copy()                                   # a padding row that receives: nobody sends its claim
    assert not rows[2][n_real + 1].any()
    rows[2][n_real + 1][c.RCV] = 1
    assert f.bad_rows(rows) == [n_real + 1] and f.verdict(rows) == 8
    # ... and with a padding row of the fold table made real that sends it, everything that row sends balanced as in
    # tests/test_fri_chip.py (the chip's zero-input padding row counted once, a padding row of the path table receiving):
    # the sums cancel, the AIRs refuse it
    n_fold = f.sh.queries * f.sh.n_rounds
    assert not rows[0][n_fold + 1].any() and not rows[3][-1][:16].any() and rows[3][-1][-1] == 0
    dig0 = rows[3][-1][F.CHIP_OUT: F.CHIP_OUT + 8]
    rows[0][n_fold + 1][F.FoldCols.REAL] = 1
    rows[0][n_fold + 1][F.FoldCols.DIG: F.FoldCols.DIG + 8] = dig0
    rows[3][-1][-1] = 1
    rows[1][-1][pc.CUR: pc.CUR + 8] = dig0
    rows[1][-1][pc.FIRST] = 1
    assert f.verdict(rows) == 3
    rows = f.copy()                                   # a real row's multiplicity taken away: its claim is received by nobody
    rows[2][f.at(q, m)][c.RCV] = 0
    assert f.bad_rows(rows) == [f.at(q, m)] and f.verdict(rows) == 8


def test_forged_claims(forge):
    f, c = forge, forge.c
    q, rd = 7, 4
    ms = [i for i, s in enumerate(f.slots) if s.rd == rd]
    lo, hi = f.at(q, ms[0]), f.at(q, ms[-1]) + f.slots[ms[-1]].width
    rows = f.copy()                                   # another X over the whole round, the table redone from it: valid in
    x = (int(f.rows[2][lo][c.X]) + 1) % P             # itself, but not the point the fold row derives from the index
    rows[2] = G.reduce_rows(f.st, points={(q, rd): x})
    assert f.bad_rows(rows) == [] and int(rows[2][lo][c.X]) == x and f.verdict(rows) == 8
    rows = f.copy()                                   # another idx over the whole round
    rows[2][lo:hi, c.IDX] = (rows[2][lo:hi, c.IDX] + 1) % P
    assert f.bad_rows(rows) == [] and f.verdict(rows) == 8
    rows = f.copy()                                   # X moved on one row in the middle of the round (the receiving row keeps its own)
    bump(rows[2][lo + 1], c.X)
    assert f.verdict(rows) == 3
    # a fold' row whose X is not shift (1 - 2 bit) x0, in a round without a matrix: the reduce table divides by nothing
    # there, so its row can carry the same X and the claim is received -- only the fold table's own constraint refuses it
    m = next(i for i, s in enumerate(f.slots) if s.matrix is None)
    rows = f.copy()
    i = q * f.sh.n_rounds + f.slots[m].rd
    bump(rows[0][i], f.fx)
    rows[2][f.at(q, m)][c.X] = rows[0][i][f.fx]
    assert f.bad_rows(rows) == [] and {r for r, _ in G.airs(f.st)[0].check_trace(rows[0], f.pubs[0])} == {i}
    assert f.verdict(rows) == 3


def test_forged_public_values(forge):
    f = forge
    m = 5
    a_at, s_at = G.reduce_public_at(m, 1)
    for at in (1, 6, a_at + 2, s_at + 1, G.reduce_public_at(1, 0)[1]):   # alpha, zeta, an A, an S of a second point, an S of a first
        pubs = [p.copy() for p in f.pubs]
        pubs[2][at] = (int(pubs[2][at]) + 1) % P
        assert f.verdict(f.rows, pubs) == 3
    for at in (G.reduce_public_at(1, 1)[0], G.reduce_public_at(1, 1)[1] + 3):   # the second point a quotient chunk does not have: must stay zero
        pubs = [p.copy() for p in f.pubs]
        assert pubs[2][at] == 0
        pubs[2][at] = 1
        assert f.verdict(f.rows, pubs) == 3


def test_verify_reduce_statement(params):
    blob, tables, init, pf = setup(params, CASES[0])
    st = G.statement(tables, pf, init, blob)
    rows = G.witness(st)
    fp = o.oracle_p3_prove(G.tables_from_rows(st, rows), st.init)
    assert G.verify_reduce_statement(tables, pf, init, fp, blob) == 0
    # a proof made for another shard proof: the same tables proven from other init words (other challenges, other openings)
    init2 = p3.to_mont([8, 6, 7])
    pf2 = o.oracle_p3_prove(tables, init2)
    st2 = G.statement(tables, pf2, init2, blob)
    fp2 = o.oracle_p3_prove(G.host_tables(st2), st2.init)
    assert G.verify_reduce_statement(tables, pf2, init2, fp2, blob) == 0
    assert G.verify_reduce_statement(tables, pf, init, fp2, blob) != 0 and G.verify_reduce_statement(tables, pf2, init2, fp, blob) != 0
    # the parent statement's proof is no proof of this one
    fst = F.statement(tables, pf, init, blob)
    assert G.verify_reduce_statement(tables, pf, init, o.oracle_p3_prove(F.host_tables(fst), fst.init), blob) != 0
    # the same statement in tables of another height (the reduce table padded to twice its rows): valid as a proof, refused by the pinned heights
    tall = rows[:2] + [np.concatenate([rows[2], np.zeros_like(rows[2])])] + rows[3:]
    ttabs = G.tables_from_rows(st, tall)
    tp = o.oracle_p3_prove(ttabs, st.init)
    assert o.oracle_p3_verify(ttabs, tp, st.init) == 0 == p3.verify(ttabs, tp, st.init, params=blob)
    assert G.verify_reduce_statement(tables, pf, init, tp, blob) == 2
    bad = pf.copy()                                   # a shard proof that is itself refused: its own reason
    bad[-3] = (int(bad[-3]) + 1) % P
    assert G.verify_reduce_statement(tables, bad, init, fp, blob) == p3.verify(tables, bad, init, params=blob) != 0
    assert not G._check_zeta(p3.to_mont([1, 2, 3, 4, 5, 0, 0, 0])) and G._check_zeta(st.in_publics)   # a zeta in the base field


def slot_words(st):
    out = []
    for s in st.slots:
        gen_n = int(p3.to_mont([pow(st.shape.root_2_27, 1 << (27 - s.log_n), P)])[0])
        out += [s.rd, s.width, s.points, s.rec_off, gen_n, int(s.last_of_round), s.row0, 0]
    return np.array(out, dtype=np.uint32)


# 301 columns: more than a workgroup takes at once; A, B: the shards of tests/test_gpu_fri_widths.py (64 / 65, 255 / 256 / 257, 513)
@pytest.mark.parametrize("case", CASES + ["sp1_width_301", "A", "B"] + PS.ROW_IDS, ids=lambda c: c if isinstance(c, str) else PS.row_id(*c))
def test_kernel_lanes_on_the_cpu(params, tmp_path, case):
    """the lane bodies of rk_fri_reduce_rows_device (p3_kernels.hpp), run as the kernels run them -- the reduce kernel's
    scans across emulated 64-lane waves (tests/emul/emul_fri_reduce.cpp) --, write the numpy witness word for word"""
    so = str(tmp_path / "libemul_fri_reduce.so")
    src = os.path.join(o.EMUL_DIR, "emul_fri_reduce.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(o.ROOT, "raiko_amd", "csrc"), "-o", so, src],
                   check=True, capture_output=True)
    lib = C.CDLL(so)
    if isinstance(case, tuple):            # a set of tests/fri_param_sets.py: fri_path_lane<0>, shiftm, wm and gen_l of another field
        blob, tables, init, pf = PS.cpu_shard(*case)
    elif case in T.FRI_SHARDS:
        blob, tables, init, pf = T.fri_setup(case, hal.make_params, o.oracle_p3_prove)
    else:
        blob, tables, init, pf = setup(params, case)
    st = G.statement(tables, pf, init, blob)
    want = [p3.to_mont(r) for r in G.witness(st)]
    rc_ext, rc_int, diag, m4 = R.tables_of()
    assert m4 == int(blob.p2_m4)
    tab = p3.to_mont(np.concatenate([rc_ext.reshape(-1), rc_int, diag]))
    got = [np.zeros_like(w) for w in want]
    sh = st.shape
    mont = lambda v: int(p3.to_mont([v])[0])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    slots, rpub = slot_words(st), st.reduce_publics
    lib.emul_fri_reduce_rows(sh.log_max, sh.blowup_log2, sh.queries, mont(pow(sh.root_2_27, 1 << (27 - sh.log_max), P)), mont(st.ext_w),
                             mont(st.coset_shift), vp(st.fold.publics), vp(st.fold.records), vp(tab), m4, len(st.slots), vp(slots),
                             G.rows_per_query(st.slots), vp(rpub), vp(st.in_records), C.c_size_t(st.per_record),
                             *[vp(g) for g in got], C.c_size_t(got[3].shape[0]))
    for g, w in zip(got, want):
        assert np.array_equal(g, w), np.argwhere(g != w)[:8]
