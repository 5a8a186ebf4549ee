"""The reduced openings of the FRI query check as a lookup table: the statement of raiko_amd.fri_chip made larger by the
part of rk_p3_verify that turns the rows a shard proof opened at a query into the values that join the fold chain.  In
fri_chip those values sit in a claims table of free cells; here a reduce table computes them and the claims table is gone.

For one query and one LDE height lh the verifier computes rop[lh] = sum_k alpha^k (p_k(x) - y_k) / (x - z_k), k over every
opened column of that height in a fixed order: the trace batch table by table (all columns at zeta, then all at
zeta gen(log_n)), then -- in a proof under a verifying key -- the preprocessed batch the same way (batch 3), then the
permutation batch the same way, then the quotient chunks at zeta.  Grouped by (matrix, point)
every group is (sum_k alpha^k p_k(x) - S) / (x - z) with S = sum_k alpha^k y_k over the same absolute powers.  S, z and the
group's first power A do not depend on the query: they are public values, recomputed from the shard proof on the host
(rk_p3_fri_inputs) as beta, the roots and the final polynomial are.  Four tables of one proof:

  fold'   fri_chip.fri_fold_air with one more column X = shift (1 - 2 bit) x0, the point of the height-(L - rd) coset at
          idx_rd; the claim it sends on BUS_FRI_CLAIM becomes (query, round, idx, X, reduced opening).
  path    fri_chip.fri_path_air, unchanged.
  reduce  fri_reduce_air: one row per (query, slot, column).  The slots of a query are the opened matrices ordered by the
          round rd = L - lh they join in (within a round: the verifier's order, which is the order of the alpha powers)
          and one single-row slot for every round without a matrix.  A row holds ONE cell P = p_k(x) that the sums of both
          points read, per point the running power (A, then x alpha along the matrix), the running sum of power x P and,
          on the matrix's last column, QUOT with QUOT (X - z) = sum - S; and the round's running reduced opening ROP.  On
          the last row of a round the row receives (query, round, idx, X, ROP) from BUS_FRI_CLAIM.  A counter pins every
          matrix to its width, a one-hot walks the slots in order and wraps to slot 0 with query + 1: no term can be
          dropped, repeated or reordered.
  chip    p3.poseidon2_chip_air.

Still free: the query indices, the opened values P (THE SEAM of this statement: raiko_amd.fri_open closes it with a sponge
over the P cells and the Merkle paths of the three input batches) and the transcript-derived public values (alpha, zeta, A, S, beta, roots,
final polynomial), which verify_reduce_statement recomputes from the shard proof and verifies the proof against.

statement / airs / witness / host_tables / device_tables / prove / verify_reduce_statement are the calls, as in fri_chip."""
import collections
import ctypes as C

import numpy as np

from . import _lib, p3
from . import fri_chip as F
from . import fri_tables as T
from .fri_chip import BUS_FRI_CLAIM, Shape
from .p3 import P, AirBuilder, ExtExpr

Matrix = collections.namedtuple("Matrix", "batch rd width points log_n")
# a row group of the reduce table: rec_off = where the matrix's opened row starts behind a record's index; row0 = its first
# row within a query; matrix = its place in the layout (None: the single row of a round without a matrix)
Slot = collections.namedtuple("Slot", "rd width points rec_off log_n last_of_round row0 matrix")


def layout_of(shape, widths, perm_widths, log_heights, lqds, prep_widths=None):
    """the layout rk_p3_fri_inputs (rk_p3_fri_inputs_key with prep_widths) reports, from the tables' widths and the proof
    header's log heights: trace, preprocessed (batch 3), permutation, quotient"""
    out = []
    for w, k in zip(widths, log_heights):
        out.append(Matrix(0, shape.log_max - k - shape.blowup_log2, w, 2, k))
    for w, k in zip(prep_widths or (), log_heights):
        if w:
            out.append(Matrix(3, shape.log_max - k - shape.blowup_log2, w, 2, k))
    for w, k in zip(perm_widths, log_heights):
        if w:
            out.append(Matrix(1, shape.log_max - k - shape.blowup_log2, w, 2, k))
    for k, lqd in zip(log_heights, lqds):
        out += [Matrix(2, shape.log_max - k - shape.blowup_log2, 4, 1, k)] * (1 << lqd)
    return out


def schedule(shape, layout):
    """the slots of one query, in row order"""
    offs = np.concatenate([[0], np.cumsum([m.width for m in layout])])
    out, row = [], 0
    for rd in range(shape.n_rounds):
        mine = [(i, m) for i, m in enumerate(layout) if m.rd == rd]
        if not mine:
            out.append(Slot(rd, 1, 0, 0, 0, True, row, None))
            row += 1
        for j, (i, m) in enumerate(mine):
            out.append(Slot(rd, m.width, m.points, int(offs[i]), m.log_n, j + 1 == len(mine), row, i))
            row += m.width
    return out


def rows_per_query(slots):
    return sum(s.width for s in slots)


class ReduceCols:
    Q, RD, IDX, X, REAL, LASTC, RCV, ENDQ, CNT, PV = range(10)
    POW, SUM, QUOT = (10, 22), (14, 26), (18, 30)         # per point, four words each
    ROP, SEL = 34, 38

    def __init__(self, n_slots):
        self.width = self.SEL + n_slots


def reduce_public_at(m, j):
    """(A, S) positions of slot m, point j in the reduce table's public values: alpha 4 | zeta 4 | per slot A0 S0 A1 S1"""
    return 8 + 16 * m + 8 * j, 8 + 16 * m + 8 * j + 4


SPONGE_COLS = 43        # PTR 8 | BUF 8 | CAP 8 | OUT 16 | FLUSH | GEND | BATCH, behind the slot one-hot (raiko_amd.fri_open)
BUS_POSEIDON2_STATE, BUS_IN_LEAF = 9, 10


def _sponge_constraints(b, c, slots, batches, pick, nsel):
    """reduce'' of raiko_amd.fri_open: the padding-free sponge of every (round, batch) group over the P cells of its rows,
    one cell per row.  batches: per slot its batch, None for the single row of a round without a matrix."""
    M = len(slots)
    loc, nxt = b.local, b.next
    PTR, BUF, CAP, OUT, FLUSH, GEND, BATCH = (c.width + k for k in (0, 8, 16, 24, 40, 41, 42))
    first, tr = b.when_first_row(), b.when_transition()
    real, lastc, pv, flush, gend = loc(c.REAL), loc(c.LASTC), loc(c.PV), loc(FLUSH), loc(GEND)
    ptr, nptr = [loc(PTR + j) for j in range(8)], [nxt(PTR + j) for j in range(8)]
    absorbs = pick([0 if bt is None else 1 for bt in batches])
    nabsorbs = F._sum([nsel[m] for m in range(M) if batches[m] is not None])
    ends = [int(batches[m] is not None and (m + 1 == M or batches[m + 1] != batches[m] or slots[m + 1].rd != slots[m].rd)) for m in range(M)]
    for v in ptr:
        b.assert_zero(v * (v - 1))
    b.assert_eq(F._sum(ptr), absorbs)                              # one position on an absorbing row, none elsewhere
    for j in range(8):
        b.assert_zero(ptr[j] * (loc(BUF + j) - pv))
    b.assert_eq(gend, lastc * pick(ends))
    b.assert_eq(loc(BATCH), pick([bt or 0 for bt in batches]))
    b.assert_eq(flush, ptr[7] + gend - ptr[7] * gend)
    # a group starts from the zero state at position 0: on the first row, behind a group end and behind the single row of
    # a round without a matrix
    start = gend + real - absorbs
    first.assert_eq(ptr[0], absorbs)
    tr.assert_zero(start * (nptr[0] - nabsorbs))
    for j in range(16):
        if j:
            first.assert_zero(loc(BUF + j))
            tr.assert_zero(start * nxt(BUF + j))                   # BUF 1..7 and CAP 0..7 (CAP follows BUF)
    cont = absorbs - flush                                         # the next row goes on in this block
    tr.assert_zero(cont * nptr[0])
    for j in range(7):
        tr.assert_zero(cont * (nptr[j + 1] - ptr[j]))
    for j in range(8):
        tr.assert_zero(cont * (1 - nptr[j]) * (nxt(BUF + j) - loc(BUF + j)))
        tr.assert_zero(cont * (nxt(CAP + j) - loc(CAP + j)))
    fl = flush - gend                                              # the next row starts the group's next block
    tr.assert_zero(fl * (nptr[0] - 1))
    for j in range(1, 16):
        tr.assert_zero(fl * (nxt(BUF + j) - loc(OUT + j)))
    return PTR, BUF, OUT, FLUSH, GEND, BATCH


def fri_reduce_air(shape, slots, ext_w=p3.EXT_W, sponge=False):
    """the reduce table (module docstring).  Every constraint has degree <= 3.  sponge: False, or the batch of every slot
    (None for the single row of a round without a matrix): reduce'' of raiko_amd.fri_open, SPONGE_COLS more columns."""
    M = len(slots)
    c = ReduceCols(M)
    b = AirBuilder(c.width + (SPONGE_COLS if sponge else 0), 8 + 16 * M, ext_w)
    loc, nxt = b.local, b.next
    ext = lambda at, f=loc: ExtExpr([f(at + k) for k in range(4)], ext_w % P)
    pub = lambda at: ExtExpr([b.public(at + k) for k in range(4)], ext_w % P)
    sel, nsel = [loc(c.SEL + m) for m in range(M)], [nxt(c.SEL + m) for m in range(M)]
    real, lastc, rcv, endq, cnt, pv = loc(c.REAL), loc(c.LASTC), loc(c.RCV), loc(c.ENDQ), loc(c.CNT), loc(c.PV)
    nreal = nxt(c.REAL)
    pick = lambda vals: F._sum([s * v for s, v in zip(sel, vals) if not (isinstance(v, int) and v == 0)] or [b.const(0)])
    for v in sel + [real, lastc]:
        b.assert_zero(v * (v - 1))
    b.assert_eq(real, F._sum(sel))
    b.assert_zero(lastc * (1 - real))
    b.assert_eq(loc(c.RD), pick([s.rd for s in slots]))
    b.assert_eq(rcv, lastc * pick([1 if s.last_of_round else 0 for s in slots]))
    b.assert_eq(endq, lastc * sel[M - 1])
    # the schedule: a table starts at (query 0, slot 0, column 0); a matrix ends where the counter reaches its width, and
    # nowhere else; the one-hot keeps or advances; after the last slot comes slot 0 of the next query, or padding for good
    first, tr = b.when_first_row(), b.when_transition()
    first.assert_eq(sel[0], b.const(1))
    first.assert_zero(loc(c.Q))
    first.assert_zero(cnt)
    b.assert_zero(lastc * (cnt - pick([s.width - 1 for s in slots])))
    tr.assert_eq(nxt(c.CNT), (real - lastc) * (cnt + 1))
    tr.assert_eq(nsel[0], (1 - lastc) * sel[0] + endq * nreal)
    for m in range(1, M):
        tr.assert_eq(nsel[m], (1 - lastc) * sel[m] + lastc * sel[m - 1])
    tr.assert_zero(nreal * (nxt(c.Q) - loc(c.Q) - endq))
    b.when_last_row().assert_eq(real, endq)
    tr.assert_zero((real - rcv) * (nxt(c.IDX) - loc(c.IDX)))       # index and point stay over a query's round
    tr.assert_zero((real - rcv) * (nxt(c.X) - loc(c.X)))
    alpha, zeta = pub(0), pub(4)
    x = ExtExpr([loc(c.X), b.const(0), b.const(0), b.const(0)], ext_w % P)
    rop, nrop = ext(c.ROP), ext(c.ROP, nxt)
    quots, nquots = [], []
    for j in range(2):
        pw, sm, qt = ext(c.POW[j]), ext(c.SUM[j]), ext(c.QUOT[j])
        npw, nsm = ext(c.POW[j], nxt), ext(c.SUM[j], nxt)
        a_of = [pub(reduce_public_at(m, j)[0]) for m in range(M)]
        s_pick = [pick([b.public(reduce_public_at(m, j)[1] + k) for m in range(M)]) for k in range(4)]
        has = pick([1 if s.points > j else 0 for s in slots])
        # the power: A on a matrix's first column, then x alpha
        start = [F._sum([nsel[m] * a_of[m].c[k] for m in range(M)]) for k in range(4)]
        step = pw * alpha
        for k in range(4):
            first.assert_eq(pw.c[k], a_of[0].c[k])
            tr.assert_eq(npw.c[k], (1 - lastc) * step.c[k] + lastc * start[k])
            # the running sum of power x P: both points read the one cell P
            first.assert_eq(sm.c[k], pw.c[k] * pv)
            tr.assert_eq(nsm.c[k], (1 - lastc) * sm.c[k] + npw.c[k] * nxt(c.PV))
        # the quotient: only on the last column of a slot that has this point, and there QUOT (X - z) = sum - S
        if j == 0:
            z = zeta
        else:
            z = zeta.scale(pick([F._gen(shape, s.log_n) if s.points > 1 else 0 for s in slots]))
        prod = qt * (x - z)
        for k in range(4):
            b.assert_zero(qt.c[k] * (1 - lastc * has))
            b.assert_zero(lastc * (prod.c[k] - sm.c[k] + s_pick[k]))
        quots.append(qt)
        nquots.append(ext(c.QUOT[j], nxt))
    for k in range(4):                                             # the round's reduced opening: starts anew behind a receiving row
        first.assert_eq(rop.c[k], quots[0].c[k] + quots[1].c[k])
        tr.assert_eq(nrop.c[k], (1 - rcv) * rop.c[k] + nquots[0].c[k] + nquots[1].c[k])
    if sponge:
        PTR, BUF, OUT, FLUSH, GEND, BATCH = _sponge_constraints(b, c, slots, list(sponge), pick, nsel)
    b.receive(BUS_FRI_CLAIM, [c.Q, c.RD, c.IDX, c.X] + list(range(c.ROP, c.ROP + 4)), mult=c.RCV, mult_is_const=False)
    if sponge:
        b.send(BUS_POSEIDON2_STATE, list(range(BUF, BUF + 32)), mult=FLUSH, mult_is_const=False)
        b.send(BUS_IN_LEAF, [c.Q, BATCH, c.RD, c.IDX] + list(range(OUT, OUT + 8)), mult=GEND, mult_is_const=False)
    return b.build()


# ---------------------------------------------------------------------------------------------- the statement
def fri_inputs(tables, proof, init=(), params=None, prep_root=None):
    """rk_p3_fri_inputs (with prep_root, the verifying key's root: rk_p3_fri_inputs_key) -> (verdict, Shape or None,
    layout [Matrix], publics, records): Montgomery words; nothing but the verdict unless it is 0"""
    rc, shape, layout, pub, rec = T.capture("rk_p3_fri_inputs", 3, tables, proof, init, params, prep_root)
    if rc != 0:
        return rc, None, None, None, None
    return 0, shape, [Matrix(*[int(v) for v in row]) for row in p3.from_mont(layout).reshape(-1, 5)], pub, rec


class Statement:
    """what the four tables state about one shard proof: fri_chip's statement (`fold`: beta, roots, final polynomial and
    the commit-phase records) and, from rk_p3_fri_inputs, the layout, alpha | zeta | A, S per matrix and point, and per
    query the index and the opened rows (Montgomery words), under `params` (None = the SP1 preset)"""

    def __init__(self, fold, layout, in_publics, in_records, params=None):
        self.fold, self.shape, self.params = fold, fold.shape, params
        self.layout = list(layout)
        self.in_publics = np.ascontiguousarray(in_publics, dtype=np.uint32)
        self.in_records = np.ascontiguousarray(in_records, dtype=np.uint32)
        self.ext_w = fold.ext_w
        self.coset_shift = int(params.coset_shift) if params is not None else 31
        self.slots = schedule(self.shape, self.layout)
        self.per_record = 1 + sum(m.width for m in self.layout)
        assert self.in_publics.size == 8 + 8 * sum(m.points for m in self.layout)
        assert self.in_records.size == self.shape.queries * self.per_record

    @property
    def layout_words(self):
        return p3.to_mont(np.array(self.layout, dtype=np.uint64).reshape(-1))

    @property
    def init(self):
        """the words the proof's transcript starts from: the shape, then the layout"""
        return np.concatenate([self.fold.init, self.layout_words])

    @property
    def reduce_publics(self):
        """alpha | zeta | per slot A0 S0 A1 S1 (zero where the slot has no such point)"""
        at = np.concatenate([[0], np.cumsum([m.points for m in self.layout])])
        out = np.zeros(8 + 16 * len(self.slots), dtype=np.uint32)
        out[:8] = self.in_publics[:8]
        for m, s in enumerate(self.slots):
            if s.matrix is not None:
                src = 8 + 8 * int(at[s.matrix])
                out[8 + 16 * m: 8 + 16 * m + 8 * s.points] = self.in_publics[src: src + 8 * s.points]
        return out


def _check_zeta(in_publics):
    """x - z must not vanish for any x of the base field: zeta (and with it zeta gen) must lie outside it"""
    return bool(np.any(np.asarray(in_publics[5:8]) != 0))


def statement(tables, proof, init=(), params=None, prep_root=None):
    """the statement about the shard proof `proof` of `tables` (raises unless rk_p3_verify accepts it; prep_root: the
    verifying key's root of a proof with preprocessed columns, rk_p3_verify_key)"""
    F._check_scope(params)
    fold = F.statement(tables, proof, init, params, prep_root)
    rc, shape, layout, pub, rec = fri_inputs(tables, proof, init, params, prep_root)
    if rc != 0 or shape != fold.shape:
        raise _lib.RkError(_lib.RK_ERR_VERIFY, "the shard proof is refused with reason %d" % rc)
    if not _check_zeta(pub):
        raise _lib.RkError(_lib.RK_ERR_INVALID, "zeta lies in the base field")
    return Statement(fold, layout, pub, rec, params)


def heights(st):
    """log heights of (fold', path, reduce, chip)"""
    h_fold, h_path, _, h_chip = F.heights(st.shape)
    return h_fold, h_path, F._log_height(st.shape.queries * rows_per_query(st.slots)), h_chip


_AIRS = {}


def airs(st):
    """(fold', path, reduce, chip) AIRs of a statement (kept per shape, schedule and parameter set)"""
    par = st.params
    addr = lambda ptr: C.cast(ptr, C.c_void_p).value
    key = (st.shape, tuple(st.slots), st.ext_w, st.coset_shift,
           None if par is None else (par.p2_m4, addr(par.p2_rc_ext), addr(par.p2_rc_int), addr(par.p2_diag)))
    if key not in _AIRS:
        _AIRS[key] = (F.fri_fold_air(st.shape, st.ext_w, coset_shift=st.coset_shift), F.fri_path_air(st.shape, st.ext_w),
                      fri_reduce_air(st.shape, st.slots, st.ext_w), p3.poseidon2_chip_air(par))
    return _AIRS[key]


def public_values(st):
    """Montgomery public values per table"""
    return [st.fold.publics, st.fold.roots, st.reduce_publics, np.zeros(0, dtype=np.uint32)]


# ---------------------------------------------------------------------------------------------- the numpy witness
def ext_inv(a, w):
    """the inverse in F_p[x] / (x^4 - w) through the tower over y = x^2: a = A + x B, 1/a = (A - x B) / (A^2 - y B^2)"""
    a0, a1, a2, a3 = [int(v) % P for v in a]
    c0 = (a0 * a0 + w * a2 * a2 - 2 * w * a1 * a3) % P           # A^2 - y B^2 = c0 + c1 y   (y^2 = w)
    c1 = (2 * a0 * a2 - a1 * a1 - w * a3 * a3) % P
    n = pow((c0 * c0 - w * c1 * c1) % P, -1, P)
    d0, d1 = c0 * n % P, -c1 * n % P                             # 1 / (c0 + c1 y)
    # (A - x B) (d0 + d1 y): A = a0 + a2 y, B = a1 + a3 y
    return [(a0 * d0 + w * a2 * d1) % P, -(a1 * d0 + w * a3 * d1) % P, (a0 * d1 + a2 * d0) % P, -(a1 * d1 + a3 * d0) % P]


def domain_point(st, idx_rd, rd):
    """the point of the height-(L - rd) coset at the (bit-reversed) position idx_rd"""
    lh = st.shape.log_max - rd
    rev = int(format(idx_rd, "0%db" % lh)[::-1], 2)
    return st.coset_shift * pow(F._gen(st.shape, lh), rev, P) % P


def reduce_rows(st, records=None, points=None):
    """canonical rows of the reduce table, padded to its height (uint64); row order: query, slot, column.  records:
    canonical (queries, per_record) records to use in place of the statement's; points: {(query, round): X} in place of
    the domain point -- what a test needs to build a table that is consistent in itself but not with the shard proof"""
    sh, w, slots = st.shape, st.ext_w, st.slots
    c = ReduceCols(len(slots))
    rpq = rows_per_query(slots)
    out = np.zeros((1 << heights(st)[2], c.width), dtype=np.uint64)
    pub = [int(v) for v in p3.from_mont(st.reduce_publics)]
    rec = p3.from_mont(st.in_records).astype(np.uint64).reshape(sh.queries, st.per_record) if records is None else records
    alpha, zeta = pub[0:4], pub[4:8]
    for q in range(sh.queries):
        idx = int(rec[q, 0])
        rop = [0, 0, 0, 0]
        for m, s in enumerate(slots):
            idx_rd = idx >> s.rd
            x = domain_point(st, idx_rd, s.rd) if points is None or (q, s.rd) not in points else points[(q, s.rd)]
            pw = [pub[reduce_public_at(m, j)[0]: reduce_public_at(m, j)[0] + 4] for j in range(2)]
            sm = [[0, 0, 0, 0], [0, 0, 0, 0]]
            for col in range(s.width):
                row = out[q * rpq + s.row0 + col]
                pv = int(rec[q, 1 + s.rec_off + col]) if s.points else 0
                last = col + 1 == s.width
                row[[c.Q, c.RD, c.IDX, c.X, c.REAL, c.LASTC, c.CNT, c.PV]] = [q, s.rd, idx_rd, x, 1, int(last), col, pv]
                row[c.SEL + m] = 1
                for j in range(2):
                    sm[j] = [(a + b * pv) % P for a, b in zip(sm[j], pw[j])]
                    row[c.POW[j]: c.POW[j] + 4], row[c.SUM[j]: c.SUM[j] + 4] = pw[j], sm[j]
                    if last and j < s.points:
                        g = F._gen(sh, s.log_n) if j else 1
                        den = [(x - zeta[0] * g) % P] + [-v * g % P for v in zeta[1:]]
                        s_at = reduce_public_at(m, j)[1]
                        quot = F._ext_mul([(a - b) % P for a, b in zip(sm[j], pub[s_at: s_at + 4])], ext_inv(den, w), w)
                        row[c.QUOT[j]: c.QUOT[j] + 4] = quot
                        rop = [(a + b) % P for a, b in zip(rop, quot)]
                    pw[j] = F._ext_mul(pw[j], alpha, w)
                row[c.ROP: c.ROP + 4] = rop
                if last:
                    row[c.RCV], row[c.ENDQ] = int(s.last_of_round), int(m + 1 == len(slots))
                    if s.last_of_round:
                        rop = [0, 0, 0, 0]
    return out


def fold_rows(st, fold):
    """fri_chip's fold rows with the column X = shift (1 - 2 bit) x0 appended"""
    fc = F.FoldCols(st.shape)
    sign = (P + 1 - 2 * fold[:, fc.BIT]) % P
    x = st.coset_shift * sign % P * fold[:, fc.X0] % P
    return np.concatenate([fold, x[:, None].astype(np.uint64)], axis=1)


def witness(st):
    """canonical rows of [fold', path, reduce, chip], padded to their heights (uint64 arrays): fri_chip's witness for the
    fold chain, the paths and the chip, the reduce table from the opened rows"""
    fold, path, _, chip = F.witness(st.fold)
    return [fold_rows(st, fold), path, reduce_rows(st), chip]


TABLE_NAMES = ("fold", "path", "reduce", "chip")


def _lead(st):
    return F._lead(st.shape) + (st.layout_words.ctypes.data_as(_lib.u32p), len(st.layout))


def device_inputs(st):
    """the four host arrays rk_fri_reduce_rows_device reads, in argument order"""
    return st.fold.publics, st.fold.records, st.reduce_publics, st.in_records


def tables_from_rows(st, rows):
    """p3 tables over canonical rows (the witness or a variation of it)"""
    return T.tables_from_rows(airs(st), rows, public_values(st))


def host_tables(st):
    """[fold', path, reduce, chip] with the numpy witness as host traces"""
    return tables_from_rows(st, witness(st))


def _pinned_tables(st):
    return T.pinned_tables(airs(st), public_values(st), heights(st))


# ---------------------------------------------------------------------------------------------- GPU rows and proof
def sizes(st):
    """rk_fri_reduce_sizes -> dict"""
    return T.sizes(_lib.RkFriReduceSizeInfo, "rk_fri_reduce_sizes", _lead(st))


def device_tables(hal, st):
    """rk_fri_reduce_rows_device under hal's parameter set -> [(DeviceBuffer, log_height)] for fold', path, reduce, chip:
    the rows stay in HBM, ready as on_device tables"""
    return T.device_tables(hal, TABLE_NAMES, sizes(st), "rk_fri_reduce_rows_device", _lead(st), device_inputs(st))


def prove(hal, st, device=None):
    """the statement's proof by rk_p3_prove over the four on_device tables (device: device_tables' result, kept by the
    caller, or None to write the rows now)"""
    return T.prove(hal, _pinned_tables(st), st.init, device if device is not None else device_tables(hal, st))


def verify_reduce_statement(tables, shard_proof, init, fri_proof, params=None, prep_root=None) -> int:
    """0 iff fri_proof proves, for shard_proof, that the reduced openings joining every query's fold chain are the ones
    rk_p3_verify computes from the rows the shard proof opened, and that the chain folds to the final polynomial.  Shape,
    layout and every public value are recomputed from the shard proof (rk_p3_fri_openings, rk_p3_fri_inputs), all four
    heights are pinned to what shape and layout give, and fri_proof is verified against them.  Otherwise the reason
    (rk_p3_verify's numbering; a shard proof that is itself refused gives its own reason; a zeta in the base field, where
    x - z could vanish, is 1).  prep_root: the verifying key's root of a shard proof with preprocessed columns (the
    captures then are the _key ones and give rk_p3_verify_key's verdict: 3 under another root, which moves every
    challenge; 5 for a preprocessed opening that does not lead to it)."""
    F._check_scope(params)
    rc, shape, pub, rec = F.fri_openings(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    rc, shape2, layout, in_pub, in_rec = fri_inputs(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    if shape2 != shape or not _check_zeta(in_pub):
        return 1
    st = Statement(F.Statement(shape, pub, rec, params), layout, in_pub, in_rec, params)
    return p3.verify(_pinned_tables(st), fri_proof, st.init, params=params)
