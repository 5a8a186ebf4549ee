"""The input-batch Merkle openings of the FRI query check as lookup tables (raiko_amd/fri_open.py, rk_p3_fri_input_paths): the
CPU side, through the oracle as tests/test_fri_reduce.py.  Honest shard proofs: roots and paths are the proof's own words
and a plain-Python replay of rk_mmcs_verify over them reaches the roots; the numpy witness satisfies all six AIRs, the
oracle proves them and both verifiers accept.  Forged statements -- each kept self-consistent apart from the one thing
named -- are proven by the oracle and refused by both verifiers with the same reason (3: a constraint, 8: a bus; the
verifier checks the cumulative sums before the constraint identity, so where both break the reason is 8).

One class of case one would want cannot exist: an injection on a path's LAST step would be a matrix whose LDE has one row, and
every table has log_n >= 1 and every parameter set blowup_log2 >= 1, so the shortest LDE has four rows and the last two
steps of every tree are plain compressions.  test_cases_exhibit_every_class asserts this bound and, in its place, an
injection on the last step at which one can occur (a two-row table: step B - 1 - (1 + blowup_log2))."""
import copy
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import field_ref as FR
import fri_param_sets as PS
import oracle_lib as o
import p2_chip_ref as R
from p3_cases import P3_CASES, init_of, tables_of
from raiko_amd import _lib, hal, p3
from raiko_amd import fri_chip as F
from raiko_amd import fri_open as H
from raiko_amd import fri_reduce as G

P = o.P
CASES = ["sp1_mixed_fib8_cubic4", "sp1_same_height", "sp1_lookup_beside_plain", "sp1_blow2_wide_k9", "sp1_width_301", "sp1_tiny_beside_tall",
         "sp1_twelve_tables"]
FORGE_CASE = "sp1_lookup_beside_plain"      # three batches, groups of 13 and 28 cells, injections in every tree


@pytest.fixture()
def params():
    yield o.oracle_set_params
    o.oracle_set_params()


_SHARDS = {}


def setup(params, case):
    """the case's shard proof, made once and shared (nothing changes it)"""
    preset, over, _, _ = P3_CASES[case]
    params(preset, **over)
    blob = hal.make_params(preset, **over)
    if case not in _SHARDS:
        tables, init = tables_of(case), init_of(case)
        _SHARDS[case] = (tables, init, o.oracle_p3_prove(tables, init))
    return (blob,) + _SHARDS[case]


def input_words_of(pf, shape, layout, log_pmax):
    """per query (trows, tpath, prows, ppath, qrows, qpath) read straight from the proof's words (the offsets of
    tests/test_fri_reduce.py opened_rows_of)"""
    L, Rn, Q = shape.log_max, shape.n_rounds, shape.queries
    trow, prow, qrow = (sum(m.width for m in layout if m.batch == b) for b in range(3))
    tail = sum(4 + 8 * (L - 1 - rd) for rd in range(Rn))
    per_query = trow + 8 * L + (prow + 8 * log_pmax if prow else 0) + qrow + 8 * L + tail
    q0 = pf.size - Q * per_query
    out = []
    for qi in range(Q):
        at = q0 + qi * per_query
        parts = []
        for n in (trow, 8 * L, prow, 8 * log_pmax if prow else 0, qrow, 8 * L):
            parts.append(pf[at: at + n])
            at += n
        out.append(parts)
    return out


def sponge_ref(cells, consts):
    """Any::hash_elems with pad_free over canonical cells"""
    s = np.zeros((1, 16), dtype=np.uint64)
    for i, v in enumerate(cells):
        s[0, i % 8] = v
        if i % 8 == 7 or i + 1 == len(cells):
            s = H._permute16(s, consts).copy()
    return [int(v) for v in s[0, :8]]


def mmcs_replay(consts, heights_log, widths, index, rows, path):
    """rk_mmcs_verify (raiko_amd/csrc/mmcs.hip) in plain Python over canonical words -> the root it reaches"""
    def level_hash(lh):
        cat, pos = [], 0
        for h, w in zip(heights_log, widths):
            if h == lh:
                cat += [int(v) for v in rows[pos: pos + w]]
            pos += w
        return sponge_ref(cat, consts) if cat else None
    B = max(heights_log)
    cur, idx = level_hash(B), index
    for lvl in range(B):
        sib = [int(v) for v in path[8 * lvl: 8 * lvl + 8]]
        pair = sib + cur if idx & 1 else cur + sib
        cur = [int(v) for v in F._permute8(np.array([pair], dtype=np.uint64), consts)[0]]
        idx >>= 1
        extra = level_hash(B - 1 - lvl)
        if extra is not None:
            cur = [int(v) for v in F._permute8(np.array([cur + extra], dtype=np.uint64), consts)[0]]
    return cur


@pytest.mark.parametrize("case", CASES)
def test_capture(params, case):
    blob, tables, init, pf = setup(params, case)
    rc, shape, roots, paths = H.fri_input_paths(tables, pf, init, blob)
    assert rc == 0 == p3.verify(tables, pf, init, params=blob)
    rc2, shape2, layout, _, rec = G.fri_inputs(tables, pf, init, blob)
    assert rc2 == 0 and shape2 == shape
    L, Q = shape.log_max, shape.queries
    log_pmax = max([m.log_n + shape.blowup_log2 for m in layout if m.batch == 1], default=0)
    assert roots.size == 25 and int(p3.from_mont(roots[24:])[0]) == log_pmax
    # the roots: the proof's words behind the header (trace), behind that the permutation root where a table has lookups
    nt = int(pf[0])
    assert np.array_equal(roots[:8], pf[1 + nt: 9 + nt])
    if log_pmax:
        assert np.array_equal(roots[8:16], pf[9 + nt: 17 + nt])
        n_perm = sum(m.batch == 1 for m in layout)
        assert np.array_equal(roots[16:24], pf[17 + nt + 4 * n_perm: 25 + nt + 4 * n_perm])
    else:
        assert not roots[8:16].any() and np.array_equal(roots[16:24], pf[9 + nt: 17 + nt])
    words = input_words_of(pf, shape, layout, log_pmax)
    per = 8 * (2 * L + log_pmax)
    recs = paths.reshape(Q, per)
    consts = F.poseidon2_tables(blob)
    rows = rec.reshape(Q, -1)
    for qi in range(Q):
        trows, tpath, prows, ppath, qrows, qpath = words[qi]
        assert np.array_equal(recs[qi], np.concatenate([tpath, ppath, qpath]))
        assert np.array_equal(rows[qi, 1:], np.concatenate([trows, prows, qrows]))
        idx = int(p3.from_mont(rows[qi, :1])[0])
        for b, rws, pth in ((0, trows, tpath), (1, prows, ppath), (2, qrows, qpath)):
            ms = [m for m in layout if m.batch == b]
            if not ms:
                continue
            hl = [m.log_n + shape.blowup_log2 for m in ms]
            got = mmcs_replay(consts, hl, [m.width for m in ms], idx >> (L - max(hl)), p3.from_mont(rws), p3.from_mont(pth))
            assert got == [int(v) for v in p3.from_mont(roots[8 * b: 8 * b + 8])], (qi, b)


def test_cases_exhibit_every_class(params):
    seen = set()
    for case in CASES:
        blob, tables, init, pf = setup(params, case)
        st = H.statement(tables, pf, init, blob)
        cells = [g.cells for g in st.groups]
        seen |= {"short"} if any(c < 8 for c in cells) else set()
        seen |= {"exact"} if any(c % 8 == 0 for c in cells) else set()
        seen |= {"partial"} if any(c > 8 and c % 8 for c in cells) else set()
        seen |= {"several"} if any(g.n_slots > 1 for g in st.groups) else set()
        hts = {t.batch: t.B for t in st.trees}
        seen |= {"short perm"} if 1 in hts and hts[1] < hts[0] else set()
        seen |= {"no perm"} if 1 not in hts else set()
        seen |= {"first step"} if any(t.group_at[0] is not None for t in st.trees) else set()
        for t in st.trees:                          # no LDE is shorter than four rows: the last two steps never inject
            assert t.group_at[-1] is None and t.group_at[-2] is None
            if t.B >= 3 + st.shape.blowup_log2 and t.group_at[t.B - 2 - st.shape.blowup_log2] is not None:
                seen.add("lowest step")             # a two-row table: the last step at which an injection can occur
        for g in st.groups:                         # the slot behind the group's last one is the single row of a round without a matrix
            nxt = g.m0 + g.n_slots
            if nxt < len(st.slots) and st.slots[nxt].matrix is None:
                seen.add("empty round behind a group end")
        seen |= {"blow-up 2"} if st.shape.blowup_log2 == 2 else set()
    assert seen == {"short", "exact", "partial", "several", "short perm", "no perm", "first step", "lowest step",
                    "empty round behind a group end", "blow-up 2"}


@pytest.mark.parametrize("case", CASES)
def test_honest_statement(params, case):
    blob, tables, init, pf = setup(params, case)
    st = H.statement(tables, pf, init, blob)
    rows = H.witness(st)
    assert [r.shape[0] for r in rows] == [1 << h for h in H.heights(st)]
    sz = H.sizes(st)
    assert tuple(sz[n + "_log_height"] for n in H.TABLE_NAMES) == H.heights(st)
    assert [sz[n + "_width"] for n in H.TABLE_NAMES] == [r.shape[1] for r in rows]
    assert (sz["n_groups"], sz["n_batches"], sz["log_pmax"], sz["paths_words"]) == (len(st.groups), len(st.trees), st.log_pmax, st.in_paths.size)
    assert sz["state_rows"] == st.shape.queries * st.perms_per_query and sz["ipath_rows"] == st.shape.queries * sum(t.B for t in st.trees)
    assert int(rows[4][:, -1].sum()) == sz["chip_rows"] and int(rows[5][:, -1].sum()) == sz["state_rows"]
    pvs = [FR.from_mont(v.astype(np.uint64)) for v in H.public_values(st)]
    for air, r, pv in zip(H.airs(st), rows, pvs):
        assert air.log_quotient_degree() == 1 and air.width == r.shape[1]
        assert air.check_trace(r, pv) == []
    tabs = H.tables_from_rows(st, rows)
    fp = o.oracle_p3_prove(tabs, st.init)
    assert o.oracle_p3_verify(tabs, fp, st.init) == 0 == p3.verify(tabs, fp, st.init, params=blob)
    assert H.verify_open_statement(tables, pf, init, fp, blob) == 0
    if case == CASES[0]:
        # the proof of the smaller statement is no proof of this one; a shard proof with one opened word changed: reason 5
        red = o.oracle_p3_prove(G.host_tables(st.red), st.red.init)
        assert H.verify_open_statement(tables, pf, init, red, blob) != 0
        words = input_words_of(pf, st.shape, st.layout, st.log_pmax)
        bad = pf.copy()
        at = (words[0][0].ctypes.data - pf.ctypes.data) // 4 + 1                  # the second opened trace word of query 0
        bad[at] = (int(bad[at]) + 1) % P
        assert p3.verify(tables, bad, init, params=blob) == 5 == H.verify_open_statement(tables, bad, init, fp, blob)
        with pytest.raises(_lib.RkError):
            H.statement(tables, bad, init, blob)


@pytest.mark.parametrize("pset,case", PS.ROW_IDS, ids=[PS.row_id(*x) for x in PS.ROW_IDS])
def test_reference_holds_under_parameter_sets(params, pset, case):
    """the oracle and the numpy witness alone under every set of tests/fri_param_sets.py"""
    st, rows = PS.check_reference(H, H.verify_open_statement, pset, case)
    sz = H.sizes(st)
    assert [r.shape[0] for r in rows] == [1 << h for h in H.heights(st)]
    assert int(rows[4][:, -1].sum()) == sz["chip_rows"] and int(rows[5][:, -1].sum()) == sz["state_rows"]
    assert any(v is not None for t in st.trees for v in t.group_at)          # a shorter matrix is injected into an input path


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.uint32).tobytes()).hexdigest()


def test_existing_airs_are_unchanged(params):
    sh = F.Shape(9, 8, 1, 10)
    layout = G.layout_of(sh, [2, 5], [0, 0], [8, 4], [0, 1])
    slots = G.schedule(sh, layout)
    a = G.fri_reduce_air(sh, slots)
    # the digest of the step list before the `sponge` argument existed
    assert sha(a.steps) == "4d9c6e6f56f2312f0b9adda1412922f2ca5238bdf6eb2aca69b46d2787f0f190" and a.width == 49 and len(a.interactions) == 1
    b = G.fri_reduce_air(sh, slots, p3.EXT_W, sponge=False)
    assert np.array_equal(a.steps, b.steps) and a.interactions[0].words() + a.interactions[0].value_cols == b.interactions[0].words() + b.interactions[0].value_cols
    s = G.fri_reduce_air(sh, slots, p3.EXT_W, sponge=H.slot_batches(layout, slots))
    assert s.width == a.width + G.SPONGE_COLS and len(s.interactions) == 3 and s.log_quotient_degree() == 1
    assert s.interactions[0].value_cols == a.interactions[0].value_cols
    c0, c8, c16 = p3.poseidon2_chip_air(None, 7), p3.poseidon2_chip_air(None, 7, n_out=8), p3.poseidon2_chip_air(None, 7, n_out=16)
    assert np.array_equal(c0.steps, c8.steps) and c0.interactions[0].words() + c0.interactions[0].value_cols == c8.interactions[0].words() + c8.interactions[0].value_cols
    # the 16-out variant: the same width and the same constraints of its own (the steps up to the first that names the
    # permutation trace or a challenge); the receive has the eight further output cells behind the others
    assert c16.width == c0.width and c16.interactions[0].value_cols[:24] == c0.interactions[0].value_cols
    assert c16.interactions[0].value_cols[16:] == list(range(c0.out_col, c0.out_col + 16))
    assert c16.interactions[0].words()[:4] == c0.interactions[0].words()[:4]
    own = next(i for i, st_ in enumerate(c0.steps.tolist()) if st_[0] in (p3.PERM_LOCAL, p3.PERM_NEXT, p3.CHALLENGE, p3.CUMSUM))
    assert own > 1000 and np.array_equal(c0.steps[:own], c16.steps[:own])
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rk_p2_chip_air_ex(None, 7, 12, C.byref(h)) == -1 and lib.rk_p2_chip_air_ex(None, 7, 16, None) == -1


def test_new_entry_points_refuse_malformed_arguments(params):
    blob, tables, init, pf = setup(params, CASES[0])
    lib = _lib.load()
    arr, keep = p3._c_tables(tables)
    n = [C.c_size_t(7), C.c_size_t(7)]
    shape = np.zeros(4, dtype=np.uint32)
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    call = lambda par, sh, a, b: lib.rk_p3_fri_input_paths(par, arr, len(tables), u(init), init.size, u(pf), pf.size, sh, None, 0, None, 0, a, b)
    assert call(C.byref(blob), None, C.byref(n[0]), C.byref(n[1])) == -1
    assert call(C.byref(blob), u(shape), None, C.byref(n[1])) == -1 and call(C.byref(blob), u(shape), C.byref(n[0]), None) == -1
    assert call(C.byref(blob), u(shape), C.byref(n[0]), C.byref(n[1])) == _lib.RK_ERR_CAPACITY and not shape.any()
    assert [v.value for v in n] == [25, 10 * 8 * 18]
    for bad in (hal.make_params(0, queries=10), hal.make_params(1, queries=10, pow_bits=7, fri_fold_log2=4),
                hal.make_params(1, queries=10, pow_bits=7, p2_pad_free=0)):
        assert call(C.byref(bad), u(shape), C.byref(n[0]), C.byref(n[1])) == -1
        with pytest.raises(_lib.RkError):
            H.statement(tables, pf, init, bad)
        with pytest.raises(_lib.RkError):
            H.verify_open_statement(tables, pf, init, pf, bad)
    del keep
    st = H.statement(tables, pf, init, blob)
    lw = st.layout_words
    out = _lib.RkFriOpenSizeInfo()
    sizes = lambda lm, bl, q, words, nm: lib.rk_fri_open_sizes(lm, bl, q, u(words) if words is not None else None, nm, C.byref(out))
    assert lib.rk_fri_open_sizes(9, 1, 10, u(lw), 5, None) == -1 and sizes(9, 1, 10, None, 5) == -1 and sizes(9, 1, 10, lw, 0) == -1
    for lm, bl, q in ((9, 0, 10), (2, 2, 10), (9, 1, 0), (10, 1, 10), (9, 2, 10)):
        assert sizes(lm, bl, q, lw, 5) == -1
    no_quotient = np.array(st.layout[:2], dtype=np.uint64).reshape(-1)          # every table is in the quotient batch
    assert sizes(9, 1, 10, p3.to_mont(no_quotient), 2) == -1
    assert sizes(9, 1, 10, lw, 5) == 0
    assert lib.rk_fri_open_rows_device(None, 9, 1, 10, u(lw), 5, *([None] * 6), *([None, 0] * 6)) == -1


# ---------------------------------------------------------------------------------------------- forged statements
class Forge:
    """the honest statement of FORGE_CASE and what a forger needs: canonical rows to vary, the verdict of both verifiers on
    the oracle's proof of a variation"""

    def __init__(self, params, pset=None):
        self.blob, self.tables, self.init, self.pf = setup(params, FORGE_CASE) if pset is None else PS.cpu_shard(pset, FORGE_CASE)
        self.st = st = H.statement(self.tables, self.pf, self.init, self.blob)
        self.rows = H.witness(st)
        self.sh, self.slots = st.shape, st.slots
        self.c, self.ic = G.ReduceCols(len(st.slots)), H.IPathCols(len(st.trees))
        S = self.c.width
        self.PTR, self.BUF, self.CAP, self.OUT, self.FLUSH, self.GEND, self.BATCH = (S + k for k in (0, 8, 16, 24, 40, 41, 42))
        self.pubs = [FR.from_mont(v.astype(np.uint64)) for v in H.public_values(st)]
        self.rec = p3.from_mont(st.red.in_records).astype(np.uint64).reshape(self.sh.queries, st.red.per_record)
        self.paths = p3.from_mont(st.in_paths).astype(np.uint64).reshape(self.sh.queries, st.per_path)
        self.rpq = G.rows_per_query(st.slots)
        self.n0 = self.sh.queries * (self.sh.n_rounds + F.steps_before(self.sh, self.sh.n_rounds))   # the chip's rows before ipath's
        self.consts = F.poseidon2_tables(self.blob)

    def copy(self):
        return [r.copy() for r in self.rows]

    def grow(self, q, gi, i=0):
        """the reduce row of query q, group gi, cell i"""
        return q * self.rpq + self.st.groups[gi].row0 + i

    def irow(self, q, k, s):
        t = self.st.trees[k]
        return t.row0 + q * t.B + s

    def chip_row_of(self, q, k, n):
        """the chip row of the n-th compression of the path (query q, tree k)"""
        t = self.st.trees[k]
        return self.n0 + t.chip0 + q * (t.B + sum(v is not None for v in t.group_at)) + n

    def state_row_of(self, q, gi, blk):
        g = self.st.groups[gi]
        return g.perms_before * self.sh.queries + q * ((g.cells + 7) // 8) + blk

    def bad_rows(self, rows, table, pubs=None):
        pubs = self.pubs if pubs is None else pubs
        return sorted({r for r, _ in H.airs(self.st)[table].check_trace(rows[table], pubs[table])})

    def verdict(self, rows, pubs=None, st=None):
        pubs = self.pubs if pubs is None else pubs
        st = self.st if st is None else st
        tabs = [p3.Table.from_canonical(a, r, pv) for a, r, pv in zip(H.airs(st), rows, pubs)]
        q = o.oracle_p3_prove(tabs, st.init)
        a, b = o.oracle_p3_verify(tabs, q, st.init), p3.verify(tabs, q, st.init, params=self.blob)
        assert a == b
        return a

    def kernel_vector(self, m, W):
        """a nonzero base-field vector d over the first five columns of slot m with sum_i alpha^i d_i = 0 in the extension:
        five unknowns, four equations.  Opened values moved by d give the same sums at both points of the matrix, hence the
        same reduced opening and the same claim: the reduce table alone cannot tell."""
        alpha = [int(v) for v in self.pubs[2][0:4]]
        cols, cur = [], [1, 0, 0, 0]
        for _ in range(5):
            cols.append(cur)
            cur = F._ext_mul(cur, alpha, W)
        A = [[cols[j][i] for j in range(5)] for i in range(4)]         # 4 x 5 over F_p
        piv = []
        r = 0
        for col in range(5):
            p_ = next((i for i in range(r, 4) if A[i][col]), None)
            if p_ is None:
                continue
            A[r], A[p_] = A[p_], A[r]
            inv = pow(A[r][col], -1, P)
            A[r] = [v * inv % P for v in A[r]]
            for i in range(4):
                if i != r and A[i][col]:
                    A[i] = [(a - A[i][col] * b) % P for a, b in zip(A[i], A[r])]
            piv.append(col)
            r += 1
        free = next(cl for cl in range(5) if cl not in piv)
        d = [0] * 5
        d[free] = 1
        for i, cl in enumerate(piv):
            d[cl] = -A[i][free] % P
        acc = [0, 0, 0, 0]
        for j in range(5):
            acc = [(a + c_ * d[j]) % P for a, c_ in zip(acc, cols[j])]
        assert acc == [0, 0, 0, 0] and any(d)
        return d


@pytest.fixture(scope="module")
def forge():
    f = Forge(o.oracle_set_params)
    yield f
    o.oracle_set_params()


@pytest.fixture(autouse=True)
def _forge_params(request):
    if "forge" in request.fixturenames:
        preset, over, _, _ = P3_CASES[FORGE_CASE]
        o.oracle_set_params(preset, **over)
    yield
    o.oracle_set_params()


def bump(row, col, by=1):
    row[col] = (int(row[col]) + by) % P


def moved_records(f):
    """opened values of query 2 moved along kernel_vector in a matrix of five or more columns: every claim stays"""
    q = 2
    gi = next(i for i, g in enumerate(f.st.groups) if g.cells >= 13)
    m = next(m for m in range(f.st.groups[gi].m0, f.st.groups[gi].m0 + f.st.groups[gi].n_slots) if f.slots[m].width >= 5)
    d = f.kernel_vector(m, int(f.blob.ext_w))
    rec = f.rec.copy()
    for j in range(5):
        bump(rec[q], 1 + f.slots[m].rec_off + j, d[j])
    touched = [q * f.rpq + f.slots[m].row0 + j for j in range(5) if d[j]]
    return q, gi, rec, touched


def test_forged_opened_values(forge):
    f = forge
    assert f.verdict(f.rows) == 0
    q, gi, rec, touched = moved_records(f)
    # opened values changed, the reduce table's own columns redone from them (same reduced openings: no claim breaks), the
    # sponge columns left as they were: only PTR (BUF - P) = 0 fails, on the rows touched
    rows = f.copy()
    rows[2][:, : f.c.width] = G.reduce_rows(f.st.red, records=rec)
    assert np.array_equal(rows[2][:, f.c.ROP: f.c.ROP + 4][rows[2][:, f.c.RCV] == 1], f.rows[2][:, f.c.ROP: f.c.ROP + 4][f.rows[2][:, f.c.RCV] == 1])
    assert f.bad_rows(rows, 2) == touched and f.verdict(rows) == 3
    # ... and with sponge, ipath, chip and state redone from them too: every table valid in itself and every bus balanced,
    # but the path of that query's batch no longer reaches the commitment: only the root constraint fails
    rows = H.witness(f.st, records=rec)
    k = next(i for i, t in enumerate(f.st.trees) if t.batch == f.st.groups[gi].batch)
    t = f.st.trees[k]
    assert [f.bad_rows(rows, i) for i in (0, 1, 2, 4, 5)] == [[]] * 5
    assert f.bad_rows(rows, 3) == [f.irow(q, k, t.B - 1)] and f.verdict(rows) == 3


def test_forged_opened_value_and_path_bit_under_the_other_matrix(params):
    """one forgery of test_forged_opened_values and one of test_forged_paths once more under m4_0: opened values moved
    with every table redone, and a path bit flipped with the path redone above it, are still refused by the root"""
    f = Forge(params, "m4_0")
    assert int(f.blob.p2_m4) == 0 and f.consts[3] == 0 and f.verdict(f.rows) == 0
    q, gi, rec, touched = moved_records(f)
    rows = H.witness(f.st, records=rec)
    k = next(i for i, t in enumerate(f.st.trees) if t.batch == f.st.groups[gi].batch)
    assert [f.bad_rows(rows, i) for i in (0, 1, 2, 4, 5)] == [[]] * 5
    assert f.bad_rows(rows, 3) == [f.irow(q, k, f.st.trees[k].B - 1)] and f.verdict(rows) == 3
    q, k, s = 3, 1, 2
    t = f.st.trees[k]
    bit = int(f.rows[3][f.irow(q, k, s)][f.ic.BIT])
    rows = H.witness(f.st, bits={(k, s, q): 1 - bit})
    assert f.bad_rows(rows, 3) == [f.irow(q, k, s), f.irow(q, k, t.B - 1)] and f.verdict(rows) == 3


def test_forged_sponge(forge):
    f = forge
    gi = next(i for i, g in enumerate(f.st.groups) if g.cells == 13)
    q = 1
    # a flush skipped: position 7 of a longer group without FLUSH (the state chip's row for it taken out of the bus): the
    # definition of FLUSH and, as the row now "goes on", the transitions behind it
    rows = f.copy()
    r = f.grow(q, gi, 7)
    assert rows[2][r][f.FLUSH] == 1 and rows[2][r][f.GEND] == 0
    rows[2][r][f.FLUSH] = 0
    rows[5][f.state_row_of(q, gi, 0)][-1] = 0
    assert f.bad_rows(rows, 2) == [r] and f.verdict(rows) == 3
    # a position advanced by two: the one-hot of cell 3 moved to position 4 (BUF[4] = P, so the row is fine in itself)
    rows = f.copy()
    r = f.grow(q, gi, 3)
    rows[2][r][f.PTR + 3], rows[2][r][f.PTR + 4], rows[2][r][f.BUF + 4] = 0, 1, rows[2][r][f.c.PV]
    assert f.bad_rows(rows, 2) == [r - 1, r] and f.verdict(rows) == 3
    # a group restarted from a nonzero state: a capacity cell set on the group's first row
    rows = f.copy()
    r = f.grow(q, gi, 0)
    rows[2][r][f.CAP + 3] = 1
    assert f.bad_rows(rows, 2) == [r - 1, r] and f.verdict(rows) == 3
    # ... and carried through the block into the state chip (input and output of that permutation redone, OUT with it, the
    # rest of the group and the path kept): the start constraint alone, at the group's first row
    rows = f.copy()
    for i in range(8):
        rows[2][f.grow(q, gi, i)][f.CAP + 3] = 1
    srow = f.state_row_of(q, gi, 0)
    sin = rows[5][srow: srow + 1, :16].copy()
    sin[0, 11] = 1
    rows[5][srow] = F.chip_rows(sin, f.consts)[0]
    rows[2][f.grow(q, gi, 7)][f.OUT: f.OUT + 16] = rows[5][srow][F.CHIP_OUT: F.CHIP_OUT + 16]
    assert f.bad_rows(rows, 2) == [r - 1, f.grow(q, gi, 7)] and f.bad_rows(rows, 5) == [] and f.verdict(rows) == 3
    # a capacity cell altered across a flush: the first row of the second block
    rows = f.copy()
    r = f.grow(q, gi, 8)
    bump(rows[2][r], f.CAP + 2)
    assert f.bad_rows(rows, 2) == [r - 1, r] and f.verdict(rows) == 3
    # GEND moved to the row before the group's end, the digest with it: the message on BUS_IN_LEAF is the same, but GEND is
    # a constant of the slot and the column -- and FLUSH follows from it
    rows = f.copy()
    e = f.grow(q, gi, 12)
    assert rows[2][e][f.GEND] == 1 and rows[2][e - 1][f.GEND] == 0
    rows[2][e][f.GEND], rows[2][e - 1][f.GEND] = 0, 1
    rows[2][e - 1][f.OUT: f.OUT + 8] = rows[2][e][f.OUT: f.OUT + 8]
    assert set(f.bad_rows(rows, 2)) == {e - 1, e} and f.verdict(rows) == 3


def without_injection(st, k, s):
    st2 = copy.copy(st)
    trees = []
    for i, t in enumerate(st.trees):
        at = [None if (i, j) == (k, s) else v for j, v in enumerate(t.group_at)]
        trees.append(t._replace(group_at=at))
    # rows and chip inputs of the trees behind it move up: as trees_of lays them out
    out, chips = [], 0
    for t in trees:
        out.append(t._replace(chip0=chips))
        chips += st.shape.queries * (t.B + sum(v is not None for v in t.group_at))
    st2.trees = out
    return st2


def last_rows(f, k):
    t = f.st.trees[k]
    return [f.irow(q, k, t.B - 1) for q in range(f.sh.queries)]


def test_forged_injections(forge):
    """a forger cannot make a path without one of its injections reach the commitment (that would be a collision), so each
    of these also misses the root on the last row of every path of that tree: the reason named is the one the verifier
    gives first, and every other constraint of every table holds"""
    f, ic = forge, forge.ic
    k = 0
    t = f.st.trees[k]
    s = max(j for j, v in enumerate(t.group_at) if v is not None)      # the tree's last injection: no other behind it
    clean = lambda rows: [f.bad_rows(rows, i) for i in (0, 1, 2, 4, 5)] == [[]] * 5
    # an injection dropped in every query, the paths redone without it: every table valid in itself, but the digests of
    # that group are sent and never received -- BUS_IN_LEAF
    st2 = without_injection(f.st, k, s)
    assert H.heights(st2) == H.heights(f.st)
    rows = H.witness(st2)
    assert clean(rows) and f.bad_rows(rows, 3) == last_rows(f, k) and f.verdict(rows) == 8
    # an injection taken one level later (RDI follows CNT there): the message received names another round and position
    st2 = copy.copy(f.st)
    at = list(t.group_at)
    assert at[s + 1] is None
    at[s], at[s + 1] = None, at[s]
    st2.trees = [t._replace(group_at=at)] + list(f.st.trees[1:])
    rows = H.witness(st2)
    assert clean(rows) and f.bad_rows(rows, 3) == last_rows(f, k) and f.verdict(rows) == 8
    # ... and with RDI as the sender has it: the level constraint RDI = L + 1 - CNT, and still the position
    for q in range(f.sh.queries):
        rows[3][f.irow(q, k, s + 1)][ic.RDI] = f.st.groups[t.group_at[s]].rd
    assert f.bad_rows(rows, 3) == sorted([f.irow(q, k, s + 1) for q in range(f.sh.queries)] + last_rows(f, k)) and f.verdict(rows) == 8
    # the arguments of the injection's compression swapped, everything above redone: the chip holds compress(ex, parent),
    # the row asks for (parent, ex -> node) -- the chip's bus
    rows = H.witness(f.st, swapped=[(k, s)])
    assert clean(rows) and f.bad_rows(rows, 3) == last_rows(f, k) and f.verdict(rows) == 8
    # ... while the same swap in one row alone, nothing redone (the chip row included): the next row's cur is not NODE
    rows = f.copy()
    r = f.irow(2, k, s)
    pair = np.concatenate([rows[3][r][ic.EX: ic.EX + 8], rows[3][r][ic.PARENT: ic.PARENT + 8]])[None, :]
    rows[3][r][ic.NODE: ic.NODE + 8] = F._permute8(pair, f.consts)[0]
    cr = f.chip_row_of(2, k, s + 1 + sum(v is not None for v in t.group_at[:s]))
    assert np.array_equal(rows[4][cr][:8], rows[3][r][ic.PARENT: ic.PARENT + 8])
    rows[4][cr] = F.chip_rows(pair, f.consts)[0]
    assert f.bad_rows(rows, 3) == [r] and f.bad_rows(rows, 4) == [] and f.verdict(rows) == 8


def test_forged_paths(forge):
    f, ic = forge, forge.ic
    q, k, s = 3, 1, 2
    t = f.st.trees[k]
    # a sibling changed, the path redone above it: only the root constraint, on that path's last row
    paths = f.paths.copy()
    bump(paths[q], t.path_off + 8 * s + 5)
    rows = H.witness(f.st, paths=paths)
    assert f.bad_rows(rows, 3) == [f.irow(q, k, t.B - 1)] and f.verdict(rows) == 3
    # a path bit flipped with POS kept, the path redone above it: POS = 2 NPOS + BIT on the flipped row, and the root
    bit = int(f.rows[3][f.irow(q, k, s)][ic.BIT])
    rows = H.witness(f.st, bits={(k, s, q): 1 - bit})
    assert f.bad_rows(rows, 3) == [f.irow(q, k, s), f.irow(q, k, t.B - 1)] and f.verdict(rows) == 3
    # ... and with nothing redone (BIT alone): the pair's order beside the position
    rows = f.copy()
    rows[3][f.irow(q, k, s)][ic.BIT] = 1 - bit
    assert f.bad_rows(rows, 3) == [f.irow(q, k, s)] and f.verdict(rows) == 3
    # an IDX that differs from the fold chain's over a whole round of one query: the claim (BUS_FRI_CLAIM) and the digests
    # (BUS_IN_LEAF) carry it, no constraint reads it
    rows = f.copy()
    rd = f.st.groups[-1].rd
    ms = [i for i, sl in enumerate(f.slots) if sl.rd == rd]
    lo, hi = q * f.rpq + f.slots[ms[0]].row0, q * f.rpq + f.slots[ms[-1]].row0 + f.slots[ms[-1]].width
    rows[2][lo:hi, f.c.IDX] = (rows[2][lo:hi, f.c.IDX] + 1) % P
    assert f.bad_rows(rows, 2) == [] and f.verdict(rows) == 8
    # a second path for the same (query, batch) in the padding rows, its compressions counted twice in the chip: the leaf
    # and the injected digests are sent once and received twice -- BUS_IN_LEAF alone
    rows = f.copy()
    n_real = f.sh.queries * sum(tr.B for tr in f.st.trees)
    assert not rows[3][n_real:].any() and rows[3].shape[0] - n_real > t.B
    rows[3][n_real: n_real + t.B] = rows[3][f.irow(q, k, 0): f.irow(q, k, 0) + t.B]
    for n in range(t.B + sum(v is not None for v in t.group_at)):
        rows[4][f.chip_row_of(q, k, n)][-1] = 2
    assert f.bad_rows(rows, 3) == [] and f.verdict(rows) == 8
    # a receiving padding row: FIRST without REAL breaks FIRST' = REAL' (1 - go), and nobody sends what it receives
    rows = f.copy()
    rows[3][n_real + 1][ic.FIRST], rows[3][n_real + 1][ic.RDF] = 1, f.sh.log_max
    assert f.bad_rows(rows, 3) == [n_real] and f.verdict(rows) == 8
    # a wrong root in the public values
    for at in (0, 8 * len(f.st.trees) - 1):
        pubs = [p.copy() for p in f.pubs]
        pubs[3][at] = (int(pubs[3][at]) + 1) % P
        assert f.verdict(f.rows, pubs) == 3


# ---------------------------------------------------------------------------------------------- the lane bodies on the CPU
def plan_words(st):
    """groups, rowinfo and levels as rk_fri_open_rows_device uploads them (p3_kernels.hpp)"""
    NONE = 0xffffffff
    groups, rowinfo = [], np.zeros(2 * G.rows_per_query(st.slots), dtype=np.uint32)
    for g in st.groups:
        groups += [g.m0, g.n_slots, g.cells, g.row0, g.perms_before, g.batch, g.rd, 0]
        for i in range(g.cells):
            rowinfo[2 * (g.row0 + i)] = i
            rowinfo[2 * (g.row0 + i) + 1] = 1 | (2 if i + 1 == g.cells else 0) | (g.batch << 2)
    levels = []
    for t in st.trees:
        lv = [NONE] * 40
        lv[:8] = [t.batch, t.B, t.row0, t.chip0, sum(v is not None for v in t.group_at), t.path_off, t.top, st.shape.log_max - t.B]
        for s, v in enumerate(t.group_at):
            if v is not None:
                lv[8 + s] = v
        levels += lv
    return np.array(groups, dtype=np.uint32), rowinfo, np.array(levels, dtype=np.uint32)


# a partial last block behind full ones (13, 28 cells) and three trees; injections on the first step of both trees
@pytest.mark.parametrize("case", ["sp1_lookup_beside_plain", "sp1_twelve_tables"] + PS.ROW_IDS, ids=lambda c: c if isinstance(c, str) else PS.row_id(*c))
def test_kernel_lanes_on_the_cpu(params, tmp_path, case):
    so = str(tmp_path / "libemul_fri_open.so")
    src = os.path.join(o.EMUL_DIR, "emul_fri_open.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(o.ROOT, "raiko_amd", "csrc"), "-o", so, src],
                   check=True, capture_output=True)
    lib = C.CDLL(so)
    blob, tables, init, pf = PS.cpu_shard(*case) if isinstance(case, tuple) else setup(params, case)   # a set: the lane bodies <0>, other tables
    st = H.statement(tables, pf, init, blob)
    if case == "sp1_twelve_tables":
        assert all(t.group_at[0] is not None for t in st.trees)
    elif case == "sp1_lookup_beside_plain":
        assert any(g.cells > 8 and g.cells % 8 for g in st.groups)
    want = [p3.to_mont(r) for r in H.witness(st)]
    rc_ext, rc_int, diag, m4 = R.tables_of()
    assert m4 == int(blob.p2_m4)
    tab = p3.to_mont(np.concatenate([rc_ext.reshape(-1), rc_int, diag]))
    sh = st.shape
    cw = G.ReduceCols(len(st.slots)).width
    reduce = want[2].copy()
    reduce[:, cw:] = 0
    ipath, chip, state = np.zeros_like(want[3]), np.zeros_like(want[4]), np.zeros_like(want[5])
    n0 = sh.queries * (sh.n_rounds + F.steps_before(sh, sh.n_rounds))
    chip_in = np.zeros((want[4].shape[0], 16), dtype=np.uint32)
    chip_mult = np.zeros(want[4].shape[0], dtype=np.uint32)
    chip_in[:n0], chip_mult[:n0] = want[4][:n0, :16], want[4][:n0, -1]
    groups, rowinfo, levels = plan_words(st)
    slots = np.array([[s.rd, s.width, s.points, s.rec_off, 0, int(s.last_of_round), s.row0, 0] for s in st.slots], dtype=np.uint32).reshape(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.emul_fri_open_rows(sh.log_max, sh.queries, len(st.slots), len(st.groups), len(st.trees), G.rows_per_query(st.slots), reduce.shape[1],
                           C.c_size_t(st.red.per_record), C.c_size_t(st.per_path), C.c_size_t(n0), vp(slots), vp(groups), vp(rowinfo), vp(levels),
                           vp(st.red.in_records), vp(st.in_paths), vp(tab), m4, vp(reduce), vp(ipath), vp(chip_in), vp(chip_mult), vp(chip),
                           C.c_size_t(chip.shape[0]), vp(state), C.c_size_t(state.shape[0]))
    for g_, w in zip((reduce, ipath, chip, state), want[2:]):
        assert np.array_equal(g_, w), np.argwhere(g_ != w)[:8]
