"""The commit phase of the FRI query check as lookup tables: one more piece of a recursion / compress layer over a
uni-stark proof (raiko_amd.p3).  For every query and every fold round of a shard proof the tables below prove that
  - the pair (folded value so far, sibling from the proof) is the leaf at idx >> 1 of that round's commit-phase tree,
  - the pair folds with that round's beta at the right domain point,
  - after the last round the result is the final polynomial
-- the part of rk_p3_verify that returns reasons 6 and 7.  Four tables of one proof, tied by lookups:

  fold    one row per (query, round): fri_fold_air.  Sends the leaf sponge (e0 | e1 | eight zeros -> digest) to the
          Poseidon2 chip, (query, round, digest, pidx) on BUS_FRI_OPEN and (query, round, idx, reduced opening) on
          BUS_FRI_CLAIM.
  path    one row per Merkle step: fri_path_air = p3.merkle_path_air's row plus a round selector (which public root the
          path must reach), the position, a step counter (the path is as long as the tree is high) and a `first` flag
          with which the row receives (query, round, cur, pos) from BUS_FRI_OPEN.
  claims  (query, round, idx, reduced opening 4, real), received from BUS_FRI_CLAIM: fri_claims_air.  THE SEAM: its rows
          are free -- a reduced-openings table and a transcript table will have to produce them.
  chip    p3.poseidon2_chip_air: one row per leaf sponge and per compression, multiplicity 1 each (no deduplication).

Public values: fold = beta of every round (4 R) | commit-phase roots (8 R) | final polynomial (4); path = the roots.
beta, roots and final polynomial are NOT derived in-STARK: verify_fri_statement recomputes them from the shard proof's
own transcript and verifies the FRI proof against them.

Scope: parameter sets with the width-16 Poseidon2 and a FRI fold by two (SP1's preset and its blowup_log2 variants).
Notation: L = log_max, R = n_rounds = L - blowup_log2, lfh(rd) = L - 1 - rd, idx_rd the query index entering round rd,
pidx = idx_rd >> 1, bit = idx_rd & 1.

statement / airs / host_tables / device_tables / prove / verify_fri_statement are the calls; host_tables is a numpy
witness of all four tables (Poseidon2 restated here), device_tables the same rows written on the GPU
(rk_fri_chip_rows_device)."""
import ctypes as C
import os
import re

import numpy as np

from . import _lib, p3
from . import fri_tables as T
from .p3 import P, AirBuilder, ExtExpr

BUS_FRI_OPEN, BUS_FRI_CLAIM = 5, 6
BUS_FRI_SAMPLE, BUS_FRI_INDEX = 11, 12      # raiko_amd.fri_transcript
SP1_ROOT_2_27, Shape = T.SP1_ROOT_2_27, T.Shape     # the shape every FRI statement carries (fri_tables)


def lfh(shape, rd):
    return shape.log_max - 1 - rd


def steps_before(shape, rd):
    """sum of lfh(r) for r < rd: the Merkle steps of one query in the rounds before rd"""
    return rd * (shape.log_max - 1) - rd * (rd - 1) // 2


def per_record(shape):
    return 1 + 8 * shape.n_rounds + 8 * steps_before(shape, shape.n_rounds)


def rec_round(shape, rd):
    return 1 + 8 * rd + 8 * steps_before(shape, rd)


def _log_height(rows):
    return max(1, int(rows - 1).bit_length())


def heights(shape):
    """log heights of (fold, path, claims, chip): they follow from the shape"""
    fold = shape.queries * shape.n_rounds
    path = shape.queries * steps_before(shape, shape.n_rounds)
    return _log_height(fold), _log_height(path), _log_height(fold), _log_height(fold + path)


# ---------------------------------------------------------------------------------------------- column plans
class FoldCols:
    Q, RD, REAL, IDX, BIT, PIDX, RO, SIB, CUR, E0, E1, FOLDED, X0, X0SQ, DIG, ZERO, SEL = 0, 1, 2, 3, 4, 5, 6, 10, 14, 18, 22, 26, 30, 31, 32, 40, 41

    def __init__(self, shape):
        self.B = self.SEL + shape.n_rounds               # bits of pidx, L - 1 of them
        self.PP = self.B + shape.log_max - 1             # partial products of x0 (round 0)
        self.width = self.PP + shape.log_max - 1


class PathCols:
    CUR, SIB, BIT, LEFT, RIGHT, PARENT, REAL, LAST, FIRST, POS, CNT, Q, RD, RSEL = 0, 8, 16, 17, 25, 33, 41, 42, 43, 44, 45, 46, 47, 48

    def __init__(self, shape):
        self.width = self.RSEL + shape.n_rounds


CLAIMS_WIDTH = 8        # query | round | idx | reduced opening 4 | real


def _sum(xs):
    t = xs[0]
    for x in xs[1:]:
        t = t + x
    return t


def _gen(shape, bits):
    return pow(shape.root_2_27, 1 << (27 - bits), P)


def fri_fold_air(shape, ext_w=p3.EXT_W, coset_shift=None, index_bus=False):
    """One row per (query, round), the rounds of a query on consecutive rows.  Enforced per row (degree <= 3):
      pair order      (e0, e1) = (cur, sib) ordered by bit; cur = the joining reduced opening in round 0, afterwards the
                      previous row's folded + this row's joining reduced opening
      fold equation   folded (-2 x0) = e0 (-2 x0) + (beta - x0)(e1 - e0)  (rk_p3_verify's fold_row cleared of the
                      inverse), beta picked from the public values by the one-hot round selector
      index           idx = 2 pidx + bit, pidx in boolean columns; the next row's bit is this row's bit 0, the bits shift down
      domain point    round 0: x0 = prod_j (1 + b_j (c_j - 1)), c_j = gen(L)^(2^(L-2-j)), through partial-product columns;
                      afterwards x0' = (1 - 2 bit') x0^2   [bitrev(2 p' + b, n) = b 2^(n-1) + bitrev(p', n-1), gen(n+1)^2 = gen(n)]
      final           in the last round folded = the public final polynomial
    and three sends with multiplicity `real` (0 on padding rows).
    coset_shift = s (raiko_amd.fri_reduce): one more column X = s (1 - 2 bit) x0 behind the others, the point of the
    height-(L - rd) coset at idx [bitrev(2 p + b, n) = b 2^(n-1) + bitrev(p, n-1), gen(n)^(2^(n-1)) = -1]; the claim sent
    becomes (query, round, idx, X, reduced opening).  None: the AIR without it.
    index_bus (raiko_amd.fri_transcript): one more column FIRST = REAL SEL[0] behind the others, with which a query's first
    row receives (query, idx) from BUS_FRI_INDEX: the index is the one the bits table cut from the transcript."""
    L, R = shape.log_max, shape.n_rounds
    nb = L - 1
    c = FoldCols(shape)
    with_x = coset_shift is not None
    first_col = c.width + (1 if with_x else 0)
    b = AirBuilder(first_col + (1 if index_bus else 0), 12 * R + 4, ext_w)
    loc, nxt = b.local, b.next
    ext = lambda at, f=loc: ExtExpr([f(at + k) for k in range(4)], ext_w % P)
    real, bit = loc(c.REAL), loc(c.BIT)
    sel, nsel = [loc(c.SEL + r) for r in range(R)], [nxt(c.SEL + r) for r in range(R)]
    bits, nbits = [loc(c.B + j) for j in range(nb)], [nxt(c.B + j) for j in range(nb)]
    for v in sel + bits + [real, bit]:
        b.assert_zero(v * (v - 1))
    b.assert_eq(real, _sum(sel))                                   # one-hot on real rows, nothing set on padding
    b.assert_zero(loc(c.ZERO))
    if R > 1:
        b.assert_eq(loc(c.RD), _sum([sel[r] * r for r in range(1, R)]))
    else:
        b.assert_zero(loc(c.RD))
    # the rounds of a query follow each other: round r is followed by round r + 1, a table starts in round 0 and ends
    # after a last round
    b.when_first_row().assert_eq(real, sel[0])
    tr = b.when_transition()
    for r in range(R - 1):
        tr.assert_eq(nsel[r + 1], sel[r])
    b.when_last_row().assert_eq(real, sel[R - 1])
    b.assert_eq(loc(c.IDX), loc(c.PIDX) * 2 + bit)
    b.assert_eq(loc(c.PIDX), _sum([bits[j] * (1 << j) for j in range(nb)]))
    cur, sib, ro, e0, e1, folded = ext(c.CUR), ext(c.SIB), ext(c.RO), ext(c.E0), ext(c.E1), ext(c.FOLDED)
    x0, x0sq = loc(c.X0), loc(c.X0SQ)
    for k in range(4):
        b.assert_zero(sel[0] * (cur.c[k] - ro.c[k]))
        b.assert_eq(e0.c[k], cur.c[k] + bit * (sib.c[k] - cur.c[k]))
        b.assert_eq(e1.c[k], sib.c[k] + bit * (cur.c[k] - sib.c[k]))
    beta = [_sum([sel[r] * b.public(4 * r + k) for r in range(R)]) for k in range(4)]
    prod = ExtExpr([beta[0] - x0] + beta[1:], ext_w % P) * (e1 - e0)
    m2x0 = x0 * (P - 2)
    for k in range(4):
        b.assert_zero((folded.c[k] - e0.c[k]) * m2x0 - prod.c[k])
        b.assert_zero(sel[R - 1] * (folded.c[k] - b.public(12 * R + k)))
    b.assert_eq(x0sq, x0 * x0)
    factor = lambda j: bits[j] * (pow(_gen(shape, L), 1 << (L - 2 - j), P) - 1) + 1
    b.assert_zero(sel[0] * (loc(c.PP) - factor(0)))
    for j in range(1, nb):
        b.assert_zero(sel[0] * (loc(c.PP + j) - loc(c.PP + j - 1) * factor(j)))
    b.assert_zero(sel[0] * (x0 - loc(c.PP + nb - 1)))
    if R > 1:
        cont = _sum(nsel[1:])                                       # the next row is a later round of the same query
        tr.assert_zero(cont * (nxt(c.Q) - loc(c.Q)))
        tr.assert_zero(cont * (nxt(c.BIT) - bits[0]))
        for j in range(nb - 1):
            tr.assert_zero(cont * (nbits[j] - bits[j + 1]))
        tr.assert_zero(cont * nbits[nb - 1])
        ncur, nro = ext(c.CUR, nxt), ext(c.RO, nxt)
        for k in range(4):
            tr.assert_zero(cont * (ncur.c[k] - folded.c[k] - nro.c[k]))
        tr.assert_zero(cont * (nxt(c.X0) - (nxt(c.BIT) * (P - 2) + 1) * x0sq))
    if with_x:
        b.assert_eq(loc(c.width), x0 * (coset_shift % P) * (1 - bit * 2))
    pair = list(range(c.E0, c.E0 + 8))
    b.send(p3.BUS_POSEIDON2, pair + [c.ZERO] * 8 + list(range(c.DIG, c.DIG + 8)), mult=c.REAL, mult_is_const=False)
    b.send(BUS_FRI_OPEN, [c.Q, c.RD] + list(range(c.DIG, c.DIG + 8)) + [c.PIDX], mult=c.REAL, mult_is_const=False)
    b.send(BUS_FRI_CLAIM, [c.Q, c.RD, c.IDX] + ([c.width] if with_x else []) + list(range(c.RO, c.RO + 4)), mult=c.REAL, mult_is_const=False)
    if index_bus:
        b.assert_eq(loc(first_col), real * sel[0])
        b.receive(BUS_FRI_INDEX, [c.Q, c.IDX], mult=first_col, mult_is_const=False)
    return b.build()


def fri_path_air(shape, ext_w=p3.EXT_W):
    """p3.merkle_path_air's row (cur 8 | sib 8 | bit | left 8 | right 8 | parent 8 | real | last) with four additions:
    a round one-hot, constant along a path, that selects which public root the last step must reach; a position with
    pos = 2 pos' + bit (pos = bit on the last step); a step counter that starts at lfh(round) and ends at 1, so that a path
    is as long as its tree is high; a `first` flag on the first step of a path with which the row receives
    (query, round, cur, pos) from BUS_FRI_OPEN.  A real step that is not the last is followed by a real step.
    Public values: the R commit-phase roots."""
    R = shape.n_rounds
    c = PathCols(shape)
    b = AirBuilder(c.width, 8 * R, ext_w)
    loc, nxt = b.local, b.next
    bit, real, last, first = loc(c.BIT), loc(c.REAL), loc(c.LAST), loc(c.FIRST)
    rsel = [loc(c.RSEL + r) for r in range(R)]
    for v in [bit, real, last, first] + rsel:
        b.assert_zero(v * (v - 1))
    b.assert_zero(last * (1 - real))
    b.assert_eq(real, _sum(rsel))
    if R > 1:
        b.assert_eq(loc(c.RD), _sum([rsel[r] * r for r in range(1, R)]))
    else:
        b.assert_zero(loc(c.RD))
    go = real * (1 - last)                                         # this path goes on in the next row
    tr = b.when_transition()
    for i in range(8):
        cur, sib = loc(c.CUR + i), loc(c.SIB + i)
        b.assert_eq(loc(c.LEFT + i), cur + bit * (sib - cur))
        b.assert_eq(loc(c.RIGHT + i), sib + bit * (cur - sib))
        tr.assert_zero(go * (nxt(c.CUR + i) - loc(c.PARENT + i)))
        b.assert_zero(last * (loc(c.PARENT + i) - _sum([rsel[r] * b.public(8 * r + i) for r in range(R)])))
    b.when_last_row().assert_zero(go)
    tr.assert_zero(go * (1 - nxt(c.REAL)))
    for r in range(R):
        tr.assert_zero(go * (nxt(c.RSEL + r) - rsel[r]))
    tr.assert_zero(go * (nxt(c.Q) - loc(c.Q)))
    pos, cnt = loc(c.POS), loc(c.CNT)
    tr.assert_zero(go * (pos - nxt(c.POS) * 2 - bit))
    b.assert_zero(last * (pos - bit))
    b.assert_zero(first * (cnt - _sum([rsel[r] * lfh(shape, r) for r in range(R)])))
    tr.assert_zero(go * (nxt(c.CNT) - cnt + 1))
    b.assert_zero(last * (cnt - 1))
    b.when_first_row().assert_eq(first, real)
    tr.assert_eq(nxt(c.FIRST), nxt(c.REAL) * (1 - go))              # a path starts wherever none is going on
    b.send(p3.BUS_POSEIDON2, list(range(c.LEFT, c.LEFT + 24)), mult=c.REAL, mult_is_const=False)
    b.receive(BUS_FRI_OPEN, [c.Q, c.RD] + list(range(c.CUR, c.CUR + 8)) + [c.POS], mult=c.FIRST, mult_is_const=False)
    return b.build()


def fri_claims_air(ext_w=p3.EXT_W):
    """(query, round, idx, reduced opening 4, real): receives every real row from BUS_FRI_CLAIM.  The rows are free; the
    only thing asserted is their order -- from one real row to the next the query number stays or goes up by one (degree 3,
    as the other three tables: one quotient shape for all four)."""
    b = AirBuilder(CLAIMS_WIDTH, 0, ext_w)
    b.assert_zero(b.local(7) * (b.local(7) - 1))
    dq = b.next(0) - b.local(0)
    b.when_transition().assert_zero(b.next(7) * dq * (dq - 1))
    b.receive(BUS_FRI_CLAIM, list(range(7)), mult=7, mult_is_const=False)
    return b.build()


# ---------------------------------------------------------------------------------------------- the statement
def _check_scope(params):
    if params is not None and (params.p2_width != 16 or params.fri_fold_log2 != 1):
        raise _lib.RkError(_lib.RK_ERR_INVALID, "the FRI tables need the width-16 Poseidon2 and a fold by two")


def fri_openings(tables, proof, init=(), params=None, prep_root=None):
    """rk_p3_fri_openings (with prep_root, the verifying key's root: rk_p3_fri_openings_key) -> (verdict, Shape or None,
    publics, records): Montgomery words; nothing but the verdict unless it is 0"""
    return T.capture("rk_p3_fri_openings", 2, tables, proof, init, params, prep_root)


_CONSTS_INC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "poseidon2_consts.inc")


def poseidon2_tables(params=None):
    """canonical (rc_ext (8, 16), rc_int (13,), diag (16,), m4) of the parameter set's width-16 instance: the arrays the
    blob names, or the library's built-in ones (csrc/poseidon2_consts.inc) where it leaves them NULL"""
    src = None

    def table(ptr, name, n):
        nonlocal src
        if params is not None and ptr:
            return p3.from_mont(np.ctypeslib.as_array(ptr, shape=(n,)).copy()).astype(np.uint64)
        if src is None:
            src = open(_CONSTS_INC).read()
        body = re.search(r"%s\[%d\]\s*=\s*\{(.*?)\}" % (name, n), src, flags=re.S).group(1)
        return p3.from_mont(np.array([int(v.rstrip("u"), 16) for v in re.findall(r"0x[0-9a-fA-F]+u?", body)], dtype=np.uint32)).astype(np.uint64)

    m4 = int(params.p2_m4) if params is not None else 1
    return (table(params and params.p2_rc_ext, "P2W16_RC_EXT_MONT", 128).reshape(8, 16), table(params and params.p2_rc_int, "P2W16_RC_INT_MONT", 13),
            table(params and params.p2_diag, "P2W16_INT_DIAG_MONT", 16), m4)


class Statement:
    """what the four tables state about one shard proof: the shape, the public values and the per-query records of
    rk_p3_fri_openings (Montgomery words), under `params` (None = the SP1 preset)"""

    def __init__(self, shape, publics, records, params=None):
        self.shape, self.params = shape, params
        self.publics = np.ascontiguousarray(publics, dtype=np.uint32)
        self.records = np.ascontiguousarray(records, dtype=np.uint32)
        self.ext_w = int(params.ext_w) if params is not None else p3.EXT_W
        assert self.publics.size == 12 * shape.n_rounds + 4 and self.records.size == shape.queries * per_record(shape)

    @property
    def roots(self):
        R = self.shape.n_rounds
        return self.publics[4 * R: 12 * R]

    @property
    def init(self):
        """the words the FRI proof's transcript starts from: the shape"""
        return p3.to_mont(list(self.shape[:4]))


def statement(tables, proof, init=(), params=None, prep_root=None):
    """the statement about the shard proof `proof` of `tables` (raises unless rk_p3_verify accepts it; prep_root: the
    verifying key's root of a proof with preprocessed columns, rk_p3_verify_key)"""
    _check_scope(params)
    rc, shape, pub, rec = fri_openings(tables, proof, init, params, prep_root)
    if rc != 0:
        raise _lib.RkError(_lib.RK_ERR_VERIFY, "the shard proof is refused with reason %d" % rc)
    return Statement(shape, pub, rec, params)


_AIRS = {}


def airs(st):
    """(fold, path, claims, chip) AIRs of a statement (kept per shape and parameter set)"""
    par = st.params
    addr = lambda ptr: C.cast(ptr, C.c_void_p).value
    key = (st.shape, st.ext_w, None if par is None else (par.p2_m4, addr(par.p2_rc_ext), addr(par.p2_rc_int), addr(par.p2_diag)))
    if key not in _AIRS:
        _AIRS[key] = (fri_fold_air(st.shape, st.ext_w), fri_path_air(st.shape, st.ext_w), fri_claims_air(st.ext_w), p3.poseidon2_chip_air(par))
    return _AIRS[key]


def public_values(st):
    """Montgomery public values per table"""
    return [st.publics, st.roots, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32)]


# ---------------------------------------------------------------------------------------------- the numpy witness
def _m_ext(c, m4):
    out = np.zeros_like(c)
    for i in range(0, 16, 4):
        a, b, d, e = (c[:, i + j] for j in range(4))
        if m4 == 0:
            rows = [(5, 7, 1, 3), (4, 6, 1, 1), (1, 3, 5, 7), (1, 1, 4, 6)]
        else:
            rows = [(2, 3, 1, 1), (1, 2, 3, 1), (1, 1, 2, 3), (3, 1, 1, 2)]
        for j, (wa, wb, wd, we) in enumerate(rows):
            out[:, i + j] = (wa * a + wb * b + wd * d + we * e) % P
    sums = (out[:, 0:4] + out[:, 4:8] + out[:, 8:12] + out[:, 12:16]) % P
    return (out + np.tile(sums, (1, 4))) % P


def chip_rows(inputs, consts, mult=None):
    """the Poseidon2 chip's rows (column order of rk_p2_chip_air, width-16 instance) for canonical inputs (n, 16):
    a restatement of the permutation that keeps the values the chip commits -> (n, 314) canonical uint64"""
    rc_ext, rc_int, diag, m4 = consts
    c = np.asarray(inputs, dtype=np.uint64) % P
    n = c.shape[0]
    cols = [c.copy()]
    cube = lambda x: x * x % P * x % P
    c = _m_ext(c, m4)

    def ext_round(c, r):
        s = (c + rc_ext[r]) % P
        x3 = cube(s)
        c = _m_ext(x3 * x3 % P * s % P, m4)
        cols.extend([x3, c.copy()])
        return c

    for r in range(4):
        c = ext_round(c, r)
    x3i, s0 = [], []
    for k in range(len(rc_int)):
        if k:
            s0.append(c[:, 0].copy())
        t = (c[:, 0] + rc_int[k]) % P
        x3 = cube(t)
        x3i.append(x3)
        c[:, 0] = x3 * x3 % P * t % P
        total = c.sum(axis=1) % P
        c = (c * diag % P + total[:, None]) % P
    cols += [np.stack(x3i, axis=1), np.stack(s0, axis=1), c.copy()]
    for r in range(4, 8):
        c = ext_round(c, r)
    cols.append((np.ones(n, dtype=np.uint64) if mult is None else np.asarray(mult, dtype=np.uint64))[:, None])
    return np.concatenate(cols, axis=1)


CHIP_OUT = 314 - 1 - 16        # the permutation's output: the state after the last external round


def _permute8(inputs, consts):
    return chip_rows(inputs, consts)[:, CHIP_OUT: CHIP_OUT + 8]


def _ext_mul(a, b, w):
    out = [0, 0, 0, 0]
    for i in range(4):
        for j in range(4):
            if i + j < 4:
                out[i + j] += a[i] * b[j]
            else:
                out[i + j - 4] += a[i] * b[j] * w
    return [v % P for v in out]


def witness(st):
    """canonical rows of the four tables, padded to their heights, from the records alone -> [fold, path, claims, chip]
    (uint64 arrays).  Row order as rk_fri_chip_rows_device writes them: fold and claims q R + rd; path round-major,
    Q steps_before(rd) + q lfh(rd) + s; chip inputs at that offset + (rd Q + q): the leaf state, then left | right of every step."""
    sh, w = st.shape, st.ext_w
    L, R, Q = sh.log_max, sh.n_rounds, sh.queries
    fc, pc = FoldCols(sh), PathCols(sh)
    h_fold, h_path, h_claims, h_chip = heights(sh)
    consts = poseidon2_tables(st.params)
    pub = [int(v) for v in p3.from_mont(st.publics)]
    rec = p3.from_mont(st.records).astype(np.uint64).reshape(Q, per_record(sh))
    fold = np.zeros((1 << h_fold, fc.width), dtype=np.uint64)
    claims = np.zeros((1 << h_claims, CLAIMS_WIDTH), dtype=np.uint64)
    path = np.zeros((1 << h_path, pc.width), dtype=np.uint64)
    chip_in = np.zeros((1 << h_chip, 16), dtype=np.uint64)
    chip_mult = np.zeros(1 << h_chip, dtype=np.uint64)
    g = _gen(sh, L)
    cj = [pow(g, 1 << (L - 2 - j), P) for j in range(L - 1)]
    for q in range(Q):
        idx = int(rec[q, 0])
        folded, x0 = [0, 0, 0, 0], 0
        for rd in range(R):
            at = rec_round(sh, rd)
            ro, sib = [int(v) for v in rec[q, at: at + 4]], [int(v) for v in rec[q, at + 4: at + 8]]
            bit, pidx = idx & 1, idx >> 1
            cur = [(a + b) % P for a, b in zip(folded, ro)] if rd else ro
            e0, e1 = (sib, cur) if bit else (cur, sib)
            row = fold[q * R + rd]
            if rd == 0:
                x0 = 1
                for j in range(L - 1):
                    if (pidx >> j) & 1:
                        x0 = x0 * cj[j] % P
                    row[fc.PP + j] = x0
            else:
                x0 = (-x0 * x0 if bit else x0 * x0) % P
            beta = pub[4 * rd: 4 * rd + 4]
            inv = pow(-2 * x0 % P, -1, P)
            slope = [(b - a) * inv % P for a, b in zip(e0, e1)]
            t = _ext_mul([(beta[0] - x0) % P] + beta[1:], slope, w)
            folded = [(a + b) % P for a, b in zip(e0, t)]
            row[[fc.Q, fc.RD, fc.REAL, fc.IDX, fc.BIT, fc.PIDX, fc.X0, fc.X0SQ]] = [q, rd, 1, idx, bit, pidx, x0, x0 * x0 % P]
            for at_col, v in ((fc.RO, ro), (fc.SIB, sib), (fc.CUR, cur), (fc.E0, e0), (fc.E1, e1), (fc.FOLDED, folded)):
                row[at_col: at_col + 4] = v
            row[fc.SEL + rd] = 1
            for j in range(lfh(sh, rd)):
                row[fc.B + j] = (pidx >> j) & 1
            claims[q * R + rd] = [q, rd, idx] + ro + [1]
            idx = pidx
    # leaves and paths, every (round, query) lane at once per step
    lanes = [(rd, q) for rd in range(R) for q in range(Q)]
    frow = np.array([q * R + rd for rd, q in lanes])
    off = np.array([Q * steps_before(sh, rd) + q * lfh(sh, rd) for rd, q in lanes])
    depth = np.array([lfh(sh, rd) for rd, _ in lanes])
    t_of = np.arange(len(lanes))
    leaf = np.concatenate([fold[frow, fc.E0: fc.E0 + 8], np.zeros((len(lanes), 8), dtype=np.uint64)], axis=1)
    chip_in[off + t_of] = leaf
    chip_mult[off + t_of] = 1
    cur = _permute8(leaf, consts)
    fold[frow, fc.DIG: fc.DIG + 8] = cur
    pos = np.array([(int(rec[q, 0]) >> rd) >> 1 for rd, q in lanes], dtype=np.uint64)
    for s in range(int(depth.max())):
        live = depth > s
        ln = np.nonzero(live)[0]
        sib = np.stack([rec[lanes[i][1], rec_round(sh, lanes[i][0]) + 8 + 8 * s: rec_round(sh, lanes[i][0]) + 16 + 8 * s] for i in ln])
        b_ = (pos[ln] & 1).astype(np.uint64)
        c_ = cur[ln]
        left = np.where(b_[:, None] == 1, sib, c_)
        right = np.where(b_[:, None] == 1, c_, sib)
        pair = np.concatenate([left, right], axis=1)
        parent = _permute8(pair, consts)
        r_ = off[ln] + s
        path[r_, pc.CUR: pc.CUR + 8] = c_
        path[r_, pc.SIB: pc.SIB + 8] = sib
        path[r_, pc.BIT] = b_
        path[r_, pc.LEFT: pc.LEFT + 16] = pair
        path[r_, pc.PARENT: pc.PARENT + 8] = parent
        path[r_, pc.REAL] = 1
        path[r_, pc.LAST] = (depth[ln] == s + 1)
        path[r_, pc.FIRST] = 1 if s == 0 else 0
        path[r_, pc.POS] = pos[ln]
        path[r_, pc.CNT] = depth[ln] - s
        path[r_, pc.Q] = [lanes[i][1] for i in ln]
        path[r_, pc.RD] = [lanes[i][0] for i in ln]
        path[r_, pc.RSEL + np.array([lanes[i][0] for i in ln])] = 1
        chip_in[off[ln] + t_of[ln] + 1 + s] = pair
        chip_mult[off[ln] + t_of[ln] + 1 + s] = 1
        cur[ln] = parent
        pos[ln] >>= np.uint64(1)
    return [fold, path, claims, chip_rows(chip_in, consts, chip_mult)]


TABLE_NAMES = ("fold", "path", "claims", "chip")


def _lead(shape):
    return shape.log_max, shape.blowup_log2, shape.queries


def device_inputs(st):
    """the two host arrays rk_fri_chip_rows_device reads, in argument order"""
    return st.publics, st.records


def tables_from_rows(st, rows):
    """p3 tables over canonical rows (the witness or a variation of it)"""
    return T.tables_from_rows(airs(st), rows, public_values(st))


def host_tables(st):
    """[fold, path, claims, chip] with the numpy witness as host traces"""
    return tables_from_rows(st, witness(st))


def _pinned_tables(st):
    return T.pinned_tables(airs(st), public_values(st), heights(st.shape))


# ---------------------------------------------------------------------------------------------- GPU rows and proof
def sizes(shape):
    """rk_fri_chip_sizes -> dict"""
    return T.sizes(_lib.RkFriChipSizeInfo, "rk_fri_chip_sizes", _lead(shape))


def device_tables(hal, st):
    """rk_fri_chip_rows_device under hal's parameter set -> [(DeviceBuffer, log_height)] for fold, path, claims, chip:
    the rows stay in HBM, ready as on_device tables"""
    return T.device_tables(hal, TABLE_NAMES, sizes(st.shape), "rk_fri_chip_rows_device", _lead(st.shape), device_inputs(st))


def prove(hal, st, device=None):
    """the FRI statement's proof by rk_p3_prove over the four on_device tables (device: device_tables' result, kept by
    the caller, or None to write the rows now)"""
    return T.prove(hal, _pinned_tables(st), st.init, device if device is not None else device_tables(hal, st))


def verify_fri_statement(tables, shard_proof, init, fri_proof, params=None, prep_root=None) -> int:
    """0 iff fri_proof proves the commit-phase checks of shard_proof: the public values (beta, roots, final polynomial)
    are recomputed from the shard proof's own transcript, all four heights are pinned to what the shape gives, and
    fri_proof is verified against them.  Otherwise the reason (rk_p3_verify's numbering; a shard proof that is itself
    refused gives its own reason).  prep_root: the verifying key's root of a shard proof with preprocessed columns."""
    _check_scope(params)
    rc, shape, pub, rec = fri_openings(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    st = Statement(shape, pub, rec, params)
    return p3.verify(_pinned_tables(st), fri_proof, st.init, params=params)
