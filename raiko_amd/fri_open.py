"""The input-batch Merkle openings of the FRI query check as lookup tables: the statement of raiko_amd.fri_reduce made larger
by the part of rk_p3_verify that returns reason 5 -- the rk_mmcs_verify calls that tie the rows a shard proof opened
at a query to its trace, permutation and quotient commitments and, under a verifying key, to the key's preprocessed
root.  In fri_reduce the opened values sit in free cells P; here
every one of them is absorbed by a sponge whose digest walks up the batch's tree to the root.  Six tables of one proof:

  fold'    as in fri_reduce, unchanged.
  path     as in fri_reduce, unchanged.
  reduce'' fri_reduce.fri_reduce_air(..., sponge=batches): the reduce row with 43 columns behind the slot one-hot,
             PTR 8 | BUF 8 | CAP 8 | OUT 16 | FLUSH | GEND | BATCH.
           fri_reduce.schedule orders a query's slots by round and, within a round, in layout order (trace matrices, then
           preprocessed (batch 3, keyed proofs), then permutation, then quotient chunks): the matrices of one
           (round, batch) GROUP -- what rk_mmcs_verify hashes
           together -- are consecutive slots in commit order, so the group's sponge absorbs a contiguous run of rows, the
           one cell P of each, in place.  PTR is the rate position P goes to (one-hot), BUF the rate cells after writing P,
           CAP the capacity, OUT the permutation's output on flush rows.  hash_elems with pad_free: a group starts from
           the zero state at position 0 (first row, behind a GEND row, behind the single row of a round without a
           matrix); PTR[j] (BUF[j] - P) = 0; without a flush the position advances by one and the other BUF cells and CAP
           stay; FLUSH = position 7 or group end; behind a flush that is no group end BUF[1..8) = OUT[1..8), CAP =
           OUT[8..16), position 0.  GEND = LASTC pick(slot ends its group) and BATCH = pick(batch) are constants of the
           slot.  Rows of a round without a matrix and padding rows have no position, hence FLUSH = GEND = 0.
           Sends (BUF | CAP | OUT) on BUS_POSEIDON2_STATE with multiplicity FLUSH and (Q, BATCH, RD, IDX, OUT[0..8)) on
           BUS_IN_LEAF with multiplicity GEND: IDX = idx >> rd is the position of the group's digest in its tree.
  ipath    fri_ipath_air: one row per (query, batch, Merkle level).  fri_chip.fri_path_air's row without the round
           (cur 8 | sib 8 | bit | left 8 | right 8 | parent 8 | real | last | first | pos | cnt | q) | BATCH | NPOS |
           INJ | EX 8 | NODE 8 | RDF | RDI | BSEL one-hot over the batches present.  A batch whose tallest LDE has log
           height B (L for trace and quotient, log_pmax for the permutation batch, log_kmax for the preprocessed batch)
           has B steps, CNT from B down to 1.  The trees are in batch-number order: the preprocessed tree (3) is last.
           parent = compress(left, right) (chip lookup, multiplicity REAL); NODE = compress(parent, EX) where INJ (chip
           lookup, multiplicity INJ; the argument order of rk_mmcs_verify) and NODE = parent elsewhere -- NODE is the
           helper that keeps "the next row's cur" and "the root on LAST" at degree 3; POS = 2 NPOS + BIT, the next row's
           POS = NPOS, NPOS = 0 on LAST.  On FIRST CNT = pick(B), RDF = L - CNT and the row receives
           (Q, BATCH, RDF, POS, CUR) from BUS_IN_LEAF; where INJ, RDI = L + 1 - CNT and it receives
           (Q, BATCH, RDI, NPOS, EX).  Public values: the roots of the batches present.
  chip     p3.poseidon2_chip_air: now also ipath's compressions.
  state    p3.poseidon2_chip_air(n_out=16) on BUS_POSEIDON2_STATE: the sponge's permutations, all 16 cells out.

Under a verifying key (statement(..., prep_root=key.root)) the opened preprocessed rows are absorbed as every other opened
row and walked up to a root that is a public value of ipath; verify_open_statement binds that value to the root the caller
trusts: the _key captures check the proof against it and hand it back as roots[25:33] (rk_p3_fri_input_paths_key).

Nothing forces INJ by a level one-hot; BUS_IN_LEAF does.  Still free: the query indices and the
transcript-derived public values (alpha, zeta, A, S, beta, the commit-phase and input roots, the final polynomial), which
verify_open_statement recomputes from the shard proof.  Scope: fri_chip's and p2_pad_free = 1.

statement / airs / witness / host_tables / device_tables / prove / verify_open_statement / sizes / heights are the calls."""
import collections
import ctypes as C

import numpy as np

from . import _lib, p3
from . import fri_chip as F
from . import fri_reduce as G
from . import fri_tables as T
from .fri_reduce import BUS_IN_LEAF, BUS_POSEIDON2_STATE, SPONGE_COLS
from .p3 import P, AirBuilder

# a (round, batch) group of one query: m0 = its first slot, row0 = its first reduce row within a query, perms_before = the
# sponge permutations of the groups before it
Group = collections.namedtuple("Group", "m0 n_slots cells row0 perms_before batch rd")
# an input tree: B = its height, group_at[s] = the group injected behind step s (None: none), top = the group its leaf is
Tree = collections.namedtuple("Tree", "batch B top group_at row0 chip0 path_off")


def _check_scope(params):
    F._check_scope(params)
    if params is not None and params.p2_pad_free != 1:
        raise _lib.RkError(_lib.RK_ERR_INVALID, "the sponge columns follow the padding-free sponge")


def slot_batches(layout, slots):
    return [None if s.matrix is None else layout[s.matrix].batch for s in slots]


def groups_of(layout, slots):
    bt = slot_batches(layout, slots)
    out, m, perms = [], 0, 0
    while m < len(slots):
        if bt[m] is None:
            m += 1
            continue
        e = m
        while e < len(slots) and bt[e] == bt[m] and slots[e].rd == slots[m].rd:
            e += 1
        cells = sum(s.width for s in slots[m:e])
        out.append(Group(m, e - m, cells, slots[m].row0, perms, bt[m], slots[m].rd))
        perms += (cells + 7) // 8
        m = e
    return out


def trees_of(shape, groups):
    out, rows, chips, path_off = [], 0, 0, 0
    for b in range(4):                                             # batch-number order: the preprocessed tree last
        mine = [(i, g) for i, g in enumerate(groups) if g.batch == b]
        B = max([shape.log_max - g.rd for _, g in mine], default=0)
        if B:
            at = [None] * B
            top = None
            for i, g in mine:
                lh = shape.log_max - g.rd
                if lh == B:
                    top = i
                else:
                    at[B - 1 - lh] = i
            out.append(Tree(b, B, top, at, rows, chips, path_off))
            rows += shape.queries * B
            chips += shape.queries * (B + sum(v is not None for v in at))
        path_off += 8 * B
    return out


class IPathCols:
    CUR, SIB, BIT, LEFT, RIGHT, PARENT, REAL, LAST, FIRST, POS, CNT, Q = 0, 8, 16, 17, 25, 33, 41, 42, 43, 44, 45, 46
    BATCH, NPOS, INJ, EX, NODE, RDF, RDI, BSEL = 47, 48, 49, 50, 58, 66, 67, 68

    def __init__(self, n_batches):
        self.width = self.BSEL + n_batches


def fri_ipath_air(shape, trees, ext_w=p3.EXT_W):
    """the input trees (module docstring); trees: [(batch, B)] of the batches present.  Every constraint has degree <= 3."""
    L, NB = shape.log_max, len(trees)
    c = IPathCols(NB)
    b = AirBuilder(c.width, 8 * NB, ext_w)
    loc, nxt = b.local, b.next
    bit, real, last, first, inj = loc(c.BIT), loc(c.REAL), loc(c.LAST), loc(c.FIRST), loc(c.INJ)
    bsel = [loc(c.BSEL + k) for k in range(NB)]
    for v in [bit, real, last, first, inj] + bsel:
        b.assert_zero(v * (v - 1))
    b.assert_zero(last * (1 - real))
    b.assert_zero(inj * (1 - real))
    b.assert_eq(real, F._sum(bsel))
    b.assert_eq(loc(c.BATCH), F._sum([bsel[k] * t[0] for k, t in enumerate(trees) if t[0]] or [b.const(0)]))
    go = real * (1 - last)                                         # this path goes on in the next row
    tr = b.when_transition()
    for i in range(8):
        cur, sib, parent, node = loc(c.CUR + i), loc(c.SIB + i), loc(c.PARENT + i), loc(c.NODE + i)
        b.assert_eq(loc(c.LEFT + i), cur + bit * (sib - cur))
        b.assert_eq(loc(c.RIGHT + i), sib + bit * (cur - sib))
        b.assert_zero((1 - inj) * (node - parent))                 # where INJ: the chip's compress(parent, ex)
        tr.assert_zero(go * (nxt(c.CUR + i) - node))
        b.assert_zero(last * (node - F._sum([bsel[k] * b.public(8 * k + i) for k in range(NB)])))
    b.when_last_row().assert_zero(go)
    tr.assert_zero(go * (1 - nxt(c.REAL)))
    for k in range(NB):
        tr.assert_zero(go * (nxt(c.BSEL + k) - bsel[k]))
    tr.assert_zero(go * (nxt(c.Q) - loc(c.Q)))
    pos, npos, cnt = loc(c.POS), loc(c.NPOS), loc(c.CNT)
    b.assert_eq(pos, npos * 2 + bit)
    tr.assert_zero(go * (nxt(c.POS) - npos))
    b.assert_zero(last * npos)
    b.assert_zero(first * (cnt - F._sum([bsel[k] * t[1] for k, t in enumerate(trees)])))
    tr.assert_zero(go * (nxt(c.CNT) - cnt + 1))
    b.assert_zero(last * (cnt - 1))
    b.assert_zero(first * (loc(c.RDF) + cnt - L))
    b.assert_zero(inj * (loc(c.RDI) + cnt - (L + 1)))
    b.when_first_row().assert_eq(first, real)
    tr.assert_eq(nxt(c.FIRST), nxt(c.REAL) * (1 - go))             # a path starts wherever none is going on
    b.send(p3.BUS_POSEIDON2, list(range(c.LEFT, c.LEFT + 24)), mult=c.REAL, mult_is_const=False)
    b.send(p3.BUS_POSEIDON2, list(range(c.PARENT, c.PARENT + 8)) + list(range(c.EX, c.EX + 16)), mult=c.INJ, mult_is_const=False)
    b.receive(BUS_IN_LEAF, [c.Q, c.BATCH, c.RDF, c.POS] + list(range(c.CUR, c.CUR + 8)), mult=c.FIRST, mult_is_const=False)
    b.receive(BUS_IN_LEAF, [c.Q, c.BATCH, c.RDI, c.NPOS] + list(range(c.EX, c.EX + 8)), mult=c.INJ, mult_is_const=False)
    return b.build()


# ---------------------------------------------------------------------------------------------- the statement
def fri_input_paths(tables, proof, init=(), params=None, prep_root=None):
    """rk_p3_fri_input_paths (with prep_root, the verifying key's root: rk_p3_fri_input_paths_key) -> (verdict, Shape or
    None, publics, records): Montgomery words; nothing but the verdict unless it is 0"""
    return T.capture("rk_p3_fri_input_paths", 2, tables, proof, init, params, prep_root)


def root_at(batch):
    """where a batch's root lies in the publics of rk_p3_fri_input_paths(_key): three roots | log_pmax | preprocessed root |
    log_kmax"""
    return 25 if batch == 3 else 8 * batch


class Statement:
    """what the six tables state about one shard proof: fri_reduce's statement (`red`) and, from rk_p3_fri_input_paths,
    the roots of the three input batches | log_pmax (| the preprocessed root | log_kmax under a verifying key) and per
    query the Merkle paths (Montgomery words)"""

    def __init__(self, red, in_roots, in_paths):
        self.red, self.fold, self.shape, self.params = red, red.fold, red.shape, red.params
        self.layout, self.slots, self.ext_w, self.coset_shift = red.layout, red.slots, red.ext_w, red.coset_shift
        self.in_roots = np.ascontiguousarray(in_roots, dtype=np.uint32)
        self.in_paths = np.ascontiguousarray(in_paths, dtype=np.uint32)
        self.batches = slot_batches(self.layout, self.slots)
        self.groups = groups_of(self.layout, self.slots)
        self.trees = trees_of(self.shape, self.groups)
        height = {t.batch: t.B for t in self.trees}
        self.roots_words = 34 if 3 in height else 25
        assert self.in_roots.size == self.roots_words, "the roots are not in the form the layout asks for"
        self.log_pmax = int(p3.from_mont(self.in_roots[24:25])[0])
        self.log_kmax = int(p3.from_mont(self.in_roots[33:34])[0]) if 3 in height else 0
        self.per_path = 8 * (2 * self.shape.log_max + self.log_pmax + self.log_kmax)
        assert self.in_paths.size == self.shape.queries * self.per_path
        assert self.log_pmax == height.get(1, 0) and self.log_kmax == height.get(3, 0)
        assert height.get(0) == self.shape.log_max and height.get(2) == self.shape.log_max and all(t.top is not None for t in self.trees)

    layout_words = property(lambda self: self.red.layout_words)
    init = property(lambda self: self.red.init)

    @property
    def ipath_publics(self):
        """the roots of the batches present"""
        return np.concatenate([self.in_roots[root_at(t.batch): root_at(t.batch) + 8] for t in self.trees])

    @property
    def perms_per_query(self):
        return sum((g.cells + 7) // 8 for g in self.groups)

    @property
    def ipath_chips_per_query(self):
        return sum(t.B + sum(v is not None for v in t.group_at) for t in self.trees)


def statement(tables, proof, init=(), params=None, prep_root=None):
    """the statement about the shard proof `proof` of `tables` (raises unless rk_p3_verify accepts it; prep_root: the
    verifying key's root of a proof with preprocessed columns, rk_p3_verify_key)"""
    _check_scope(params)
    red = G.statement(tables, proof, init, params, prep_root)
    rc, shape, roots, paths = fri_input_paths(tables, proof, init, params, prep_root)
    if rc != 0 or shape != red.shape:
        raise _lib.RkError(_lib.RK_ERR_VERIFY, "the shard proof is refused with reason %d" % rc)
    return Statement(red, roots, paths)


def heights(st):
    """log heights of (fold', path, reduce'', ipath, chip, state)"""
    h_fold, h_path, h_reduce, _ = G.heights(st.red)
    sh = st.shape
    chip = sh.queries * (sh.n_rounds + F.steps_before(sh, sh.n_rounds) + st.ipath_chips_per_query)
    return (h_fold, h_path, h_reduce, F._log_height(sh.queries * sum(t.B for t in st.trees)), F._log_height(chip),
            F._log_height(sh.queries * st.perms_per_query))


def _roots_bound(roots, prep_root):
    """the preprocessed root among the captured roots is the caller's, word for word (and there is none without one)"""
    if prep_root is None:
        return roots.size == 25
    return roots.size == 34 and np.array_equal(roots[25:33], np.ascontiguousarray(prep_root, dtype=np.uint32).reshape(-1))


_AIRS = {}


def airs(st):
    """(fold', path, reduce'', ipath, chip, state) AIRs of a statement (kept per shape, schedule and parameter set)"""
    par = st.params
    addr = lambda ptr: C.cast(ptr, C.c_void_p).value
    key = (st.shape, tuple(st.slots), tuple(st.batches), st.ext_w, st.coset_shift,
           None if par is None else (par.p2_m4, addr(par.p2_rc_ext), addr(par.p2_rc_int), addr(par.p2_diag)))
    if key not in _AIRS:
        _AIRS[key] = (F.fri_fold_air(st.shape, st.ext_w, coset_shift=st.coset_shift), F.fri_path_air(st.shape, st.ext_w),
                      G.fri_reduce_air(st.shape, st.slots, st.ext_w, sponge=st.batches),
                      fri_ipath_air(st.shape, [(t.batch, t.B) for t in st.trees], st.ext_w), p3.poseidon2_chip_air(par),
                      p3.poseidon2_chip_air(par, BUS_POSEIDON2_STATE, n_out=16))
    return _AIRS[key]


def public_values(st):
    """Montgomery public values per table"""
    none = np.zeros(0, dtype=np.uint32)
    return [st.fold.publics, st.fold.roots, st.red.reduce_publics, st.ipath_publics, none, none]


# ---------------------------------------------------------------------------------------------- the numpy witness
def _permute16(inputs, consts):
    return F.chip_rows(inputs, consts)[:, F.CHIP_OUT: F.CHIP_OUT + 16]


def sponge_rows(st, reduce, consts, records=None):
    """the sponge columns of reduce'' over the P cells of `reduce` (canonical rows of the reduce table, padded) ->
    (reduce'' rows, state chip inputs, their multiplicities, digests (queries, groups, 8))"""
    sh = st.shape
    Q, rpq = sh.queries, G.rows_per_query(st.slots)
    S = reduce.shape[1]
    out = np.concatenate([reduce, np.zeros((reduce.shape[0], SPONGE_COLS), dtype=np.uint64)], axis=1)
    PTR, BUF, CAP, OUT, FLUSH, GEND, BATCH = (S + k for k in (0, 8, 16, 24, 40, 41, 42))
    n_state = 1 << heights(st)[5]
    sin, smult = np.zeros((n_state, 16), dtype=np.uint64), np.zeros(n_state, dtype=np.uint64)
    dig = np.zeros((Q, len(st.groups), 8), dtype=np.uint64)
    qrow = np.arange(Q) * rpq
    for gi, g in enumerate(st.groups):
        state = np.zeros((Q, 16), dtype=np.uint64)
        n_perm = (g.cells + 7) // 8
        for i in range(g.cells):
            r = qrow + g.row0 + i
            pos, end = i % 8, i + 1 == g.cells
            state[:, pos] = out[r, G.ReduceCols.PV]
            out[r, PTR + pos] = 1
            out[r, BUF: BUF + 16] = state
            out[r, GEND], out[r, BATCH] = int(end), g.batch
            if pos == 7 or end:
                srow = g.perms_before * Q + np.arange(Q) * n_perm + i // 8
                sin[srow], smult[srow] = state, 1
                state = _permute16(state, consts).copy()
                out[r, OUT: OUT + 16] = state
                out[r, FLUSH] = 1
        dig[:, gi] = state[:, :8]
    return out, sin, smult, dig


def ipath_rows(st, dig, consts, paths=None, bits=None, swapped=()):
    """canonical rows of ipath, padded, and the chip inputs of its compressions in row order of the chip table behind the
    commit-phase ones -> (rows, chip inputs (n, 16)); dig: sponge_rows' digests; paths: canonical (queries, per_path).
    What a test needs to build paths that are consistent in themselves but wrong: bits = {(tree, step, query): bit} orders
    that step's pair by another bit than the position's; swapped = [(tree, step)] injects compress(ex, parent) there."""
    sh = st.shape
    L, Q = sh.log_max, sh.queries
    c = IPathCols(len(st.trees))
    rows = np.zeros((1 << heights(st)[3], c.width), dtype=np.uint64)
    cin = np.zeros((Q * st.ipath_chips_per_query, 16), dtype=np.uint64)
    paths = p3.from_mont(st.in_paths).astype(np.uint64).reshape(Q, st.per_path) if paths is None else paths
    idx = p3.from_mont(st.red.in_records.reshape(Q, st.red.per_record)[:, 0]).astype(np.uint64)
    qs = np.arange(Q)
    for k, t in enumerate(st.trees):
        n_inj = sum(v is not None for v in t.group_at)
        pos = idx >> np.uint64(L - t.B)
        cur = dig[:, t.top].copy()
        chip = t.chip0 + qs * (t.B + n_inj)
        for s in range(t.B):
            r = t.row0 + qs * t.B + s
            sib = paths[:, t.path_off + 8 * s: t.path_off + 8 * s + 8]
            bit = (pos & np.uint64(1)).astype(np.uint64)
            for (k_, s_, q_), v in (bits or {}).items():
                if (k_, s_) == (k, s):
                    bit[q_] = v
            left = np.where(bit[:, None] == 1, sib, cur)
            right = np.where(bit[:, None] == 1, cur, sib)
            pair = np.concatenate([left, right], axis=1)
            parent = F._permute8(pair, consts)
            cin[chip] = pair
            chip = chip + 1
            cnt = t.B - s
            rows[r, c.CUR: c.CUR + 8], rows[r, c.SIB: c.SIB + 8], rows[r, c.BIT] = cur, sib, bit
            rows[r, c.LEFT: c.LEFT + 16], rows[r, c.PARENT: c.PARENT + 8] = pair, parent
            rows[r, c.REAL], rows[r, c.LAST], rows[r, c.FIRST] = 1, int(s + 1 == t.B), int(s == 0)
            rows[r, c.POS], rows[r, c.CNT], rows[r, c.Q], rows[r, c.BATCH], rows[r, c.NPOS] = pos, cnt, qs, t.batch, pos >> np.uint64(1)
            rows[r, c.BSEL + k] = 1
            node = parent
            if t.group_at[s] is not None:
                ex = dig[:, t.group_at[s]]
                pair = np.concatenate([ex, parent] if (k, s) in swapped else [parent, ex], axis=1)
                node = F._permute8(pair, consts)
                cin[chip] = pair
                chip = chip + 1
                rows[r, c.INJ], rows[r, c.EX: c.EX + 8], rows[r, c.RDI] = 1, ex, L + 1 - cnt
            rows[r, c.NODE: c.NODE + 8] = node
            if s == 0:
                rows[r, c.RDF] = L - cnt
            cur, pos = node, pos >> np.uint64(1)
    return rows, cin


def witness(st, records=None, paths=None, bits=None, swapped=()):
    """canonical rows of [fold', path, reduce'', ipath, chip, state], padded to their heights (uint64 arrays).  records /
    paths: canonical opened rows (queries, per_record) / paths (queries, per_path) to use in place of the statement's:
    what a test needs to build tables that are consistent in themselves but not with the shard proof (bits, swapped:
    ipath_rows)"""
    sh = st.shape
    consts = F.poseidon2_tables(st.params)
    fold, path, _, chip = F.witness(st.fold)
    reduce, sin, smult, dig = sponge_rows(st, G.reduce_rows(st.red, records=records), consts)
    ipath, cin = ipath_rows(st, dig, consts, paths, bits, swapped)
    n0 = sh.queries * (sh.n_rounds + F.steps_before(sh, sh.n_rounds))
    n_chip = 1 << heights(st)[4]
    more = F.chip_rows(cin, consts)
    pad = F.chip_rows(np.zeros((1, 16), dtype=np.uint64), consts, [0])
    chip = np.concatenate([chip[:n0], more, np.repeat(pad, n_chip - n0 - more.shape[0], axis=0)])
    return [G.fold_rows(st.red, fold), path, reduce, ipath, chip, F.chip_rows(sin, consts, smult)]


TABLE_NAMES = ("fold", "path", "reduce", "ipath", "chip", "state")


def device_inputs(st):
    """the six host arrays rk_fri_open_rows_device reads, in argument order"""
    return (st.fold.publics, st.fold.records, st.red.reduce_publics, st.red.in_records, st.in_roots, st.in_paths)


def tables_from_rows(st, rows):
    """p3 tables over canonical rows (the witness or a variation of it)"""
    return T.tables_from_rows(airs(st), rows, public_values(st))


def host_tables(st):
    """the six tables with the numpy witness as host traces"""
    return tables_from_rows(st, witness(st))


def _pinned_tables(st):
    return T.pinned_tables(airs(st), public_values(st), heights(st))


# ---------------------------------------------------------------------------------------------- GPU rows and proof
def sizes(st):
    """rk_fri_open_sizes -> dict.  The row writer cannot tell a 25-word d_roots from the 34-word form a layout with a
    preprocessed batch needs: the statement's roots must be what the plan reports."""
    sz = T.sizes(_lib.RkFriOpenSizeInfo, "rk_fri_open_sizes", G._lead(st))
    assert sz["roots_words"] == st.in_roots.size and sz["log_kmax"] == st.log_kmax
    return sz


def device_tables(hal, st):
    """rk_fri_open_rows_device under hal's parameter set -> [(DeviceBuffer, log_height)] for the six tables: the rows stay
    in HBM, ready as on_device tables"""
    return T.device_tables(hal, TABLE_NAMES, sizes(st), "rk_fri_open_rows_device", G._lead(st), device_inputs(st))


def prove(hal, st, device=None):
    """the statement's proof by rk_p3_prove over the six on_device tables (device: device_tables' result, kept by the
    caller, or None to write the rows now)"""
    return T.prove(hal, _pinned_tables(st), st.init, device if device is not None else device_tables(hal, st))


def verify_open_statement(tables, shard_proof, init, fri_proof, params=None, prep_root=None) -> int:
    """0 iff fri_proof proves, for shard_proof, what verify_reduce_statement states and that every opened value the reduced
    openings are computed from lies in the tree of its batch's commitment.  Shape, layout, every public value, the roots
    and the records are recomputed from the shard proof (rk_p3_fri_openings, rk_p3_fri_inputs, rk_p3_fri_input_paths), all
    six heights are pinned to what shape and layout give, and fri_proof is verified against them.  Otherwise the reason
    (rk_p3_verify's numbering, as verify_reduce_statement).  prep_root: the verifying key's root of a shard proof with
    preprocessed columns: the root the caller trusts.  The captures check the shard proof against it (refused under
    another root) and the ipath table's public value for the preprocessed tree is that root."""
    _check_scope(params)
    rc, shape, pub, rec = F.fri_openings(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    rc, shape2, layout, in_pub, in_rec = G.fri_inputs(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    rc, shape3, roots, paths = fri_input_paths(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    if shape2 != shape or shape3 != shape or not G._check_zeta(in_pub):
        return 1
    if not _roots_bound(roots, prep_root):
        return 1
    st = Statement(G.Statement(F.Statement(shape, pub, rec, params), layout, in_pub, in_rec, params), roots, paths)
    return p3.verify(_pinned_tables(st), fri_proof, st.init, params=params)
