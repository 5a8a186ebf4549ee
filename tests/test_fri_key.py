"""The FRI query check of proofs under a verifying key (rk_p3_verify_hashes_key, the four rk_p3_fri_*_key captures, the
plans of rk_fri_{reduce,open,transcript}_sizes over a layout with a fourth batch, and the three Python statements with
prep_root): the CPU side, over the committed keyed proofs of tests/golden/p3-prep (preset 1, queries=7, pow_bits=2).
range_prep: four tables, lookups and a preprocessed table shorter than the tallest -- four trees, log_kmax < log_max.
gate_next: one table without lookups -- three trees, the preprocessed one at full height.  The statements' own tables have
no preprocessed columns, so the oracle proves them as in tests/test_fri_open.py; forged statements are kept self-consistent
apart from the one thing named and refused for that reason (3: a constraint, 8: a bus)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import field_ref as FR
import oracle_lib as o
import p2_chip_ref as R
import p3_prep_cases as K
import p3_ref_prep as RP
from p3_cases import P3_CASES, init_of, tables_of
from test_fri_open import plan_words
from raiko_amd import _lib, hal, p3
from raiko_amd import fri_chip as F
from raiko_amd import fri_open as H
from raiko_amd import fri_reduce as G
from raiko_amd import fri_tables as T
from raiko_amd import fri_transcript as X

P = o.P
GOLDEN = os.path.join(o.ROOT, "tests", "golden", "p3-prep")
OVER = dict(queries=7, pow_bits=2)
INVALID, CAPACITY = _lib.RK_ERR_INVALID, _lib.RK_ERR_CAPACITY
CAPTURES = (("rk_p3_fri_openings", 2), ("rk_p3_fri_inputs", 3), ("rk_p3_fri_input_paths", 2), ("rk_p3_fri_transcript", 3))
UNKEYED_CASE = "sp1_lookup_beside_plain"


class Fixture:
    def __init__(self, name):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        if name == "range_prep":
            cpu, add, mul, _ = p3.lookup_demo_airs()
            airs = [cpu, add, mul, p3.p3_range_air_prep()]
        else:
            airs = [K.gate_air(2, True)]
        self.name = name
        self.full = [p3.Table(a, z["trace%d" % i], (), prep=z["prep%d" % i] if "prep%d" % i in z.files else None) for i, a in enumerate(airs)]
        self.tables = K.pinned(self.full)
        self.pf, self.root, self.init = z["proof"], z["root"], z["init"]
        self.par = hal.make_params(1, **OVER)
        self.args = (self.tables, self.pf, self.init, self.par)
        self._st = None

    @property
    def st(self):
        """the transcript statement (it holds the open and the reduce statement), made once"""
        if self._st is None:
            self._st = X.statement(*self.args, prep_root=self.root)
        return self._st

    def other_root(self, word=3):
        bad = self.root.copy()
        bad[word] = (int(bad[word]) + 1) % P
        return bad


_FX = {}


@pytest.fixture(params=["range_prep", "gate_next"])
def fx(request):
    o.oracle_set_params(1, **OVER)
    if request.param not in _FX:
        _FX[request.param] = Fixture(request.param)
    yield _FX[request.param]
    o.oracle_set_params()


@pytest.fixture()
def rp():
    o.oracle_set_params(1, **OVER)
    if "range_prep" not in _FX:
        _FX["range_prep"] = Fixture("range_prep")
    yield _FX["range_prep"]
    o.oracle_set_params()


def canon(a):
    return FR.from_mont(np.asarray(a).astype(np.uint64))


# ---------------------------------------------------------------------------------------------- the captures
def test_key_captures(fx):
    tables, pf, init, par = fx.args
    assert p3.verify(tables, pf, init, params=par, prep_root=fx.root) == 0
    rc, shape, pub, rec = F.fri_openings(*fx.args, prep_root=fx.root)
    rc2, shape2, layout, in_pub, in_rec = G.fri_inputs(*fx.args, prep_root=fx.root)
    rc3, shape3, roots, paths = H.fri_input_paths(*fx.args, prep_root=fx.root)
    rc4, shape4, ops, obs, smp = X.fri_transcript(*fx.args, prep_root=fx.root)
    assert (rc, rc2, rc3, rc4) == (0, 0, 0, 0) and shape == shape2 == shape3 == shape4
    L, Q, blow = shape.log_max, shape.queries, shape.blowup_log2
    assert Q == OVER["queries"]
    # the layout: trace, preprocessed (3), permutation, quotient, by table in each, with the tables' widths
    log_n = [int(v) for v in pf[1: 1 + len(tables)]]
    want = G.layout_of(shape, [t.air.width for t in tables], [t.air.perm_width for t in tables], log_n,
                       [t.air.log_quotient_degree() for t in tables], prep_widths=[t.air.prep_width for t in tables])
    assert layout == want
    order = [m.batch for m in layout]
    assert order == sorted(order, key=(0, 3, 1, 2).index) and 3 in order and order[0] == 0
    assert all(m.points == 2 for m in layout if m.batch == 3)
    trow, prow, qrow, krow = (sum(m.width for m in layout if m.batch == b) for b in range(4))
    log_pmax = max([m.log_n + blow for m in layout if m.batch == 1], default=0)
    log_kmax = max(m.log_n + blow for m in layout if m.batch == 3)
    assert (log_kmax < L) == (fx.name == "range_prep") and (log_pmax > 0) == (fx.name == "range_prep")
    # the sizes of a record
    assert in_rec.size == Q * (1 + trow + krow + prow + qrow)
    assert paths.size == Q * 8 * (2 * L + log_pmax + log_kmax)
    assert in_pub.size == 8 + 8 * sum(m.points for m in layout)
    # the paths publics: the 25 words of the three-batch form, then the caller's root and log_kmax
    assert roots.size == 34 and np.array_equal(roots[25:33], fx.root) and int(canon(roots[33:])[0]) == log_kmax
    assert int(canon(roots[24:25])[0]) == log_pmax
    nt = len(tables)
    assert np.array_equal(roots[:8], pf[1 + nt: 9 + nt])
    # the inputs and paths records against the words the exact reference reads from the proof
    spans = RP.parse(fx.full, pf, blow, Q)["spans"]
    recs, pths = in_rec.reshape(Q, -1), paths.reshape(Q, -1)
    for q in range(Q):
        cut = lambda name: pf[slice(*spans["q%d.%s" % (q, name)])] if "q%d.%s" % (q, name) in spans else pf[:0]
        assert np.array_equal(recs[q, 1:], np.concatenate([cut("trace_rows"), cut("prep_rows"), cut("perm_rows"), cut("quotient_rows")]))
        assert np.array_equal(pths[q], np.concatenate([cut("trace_path"), cut("perm_path"), cut("quotient_path"), cut("prep_path")]))
        assert cut("prep_rows").size == krow and cut("prep_path").size == 8 * log_kmax
    # the transcript: init | root | trace root
    n = init.size
    assert np.array_equal(obs[:n], init) and np.array_equal(obs[n: n + 8], fx.root) and np.array_equal(obs[n + 8: n + 16], roots[:8])
    assert [tuple(int(v) for v in x) for x in canon(ops).reshape(-1, 2)[:3]] == [(0, n), (0, 8), (0, 8)]


def test_key_hashes(fx):
    """rk_p3_verify_hashes_key: every permutation of the keyed check is one the transcript statement's chip or state
    chip proves -- the counts agree -- and the first permutations absorb init | root"""
    rc, states = p3.verify_hashes(*fx.args, prep_root=fx.root)
    assert rc == 0
    sz = X.sizes(fx.st)
    assert states.shape == (sz["chip_rows"] + sz["state_rows"], 16)
    head = np.concatenate([fx.init, fx.root])
    assert np.array_equal(states[0, : min(8, head.size)], head[:8])
    assert np.array_equal(states[1, : head.size - 8], head[8:])
    # every input of the two chip tables, as a multiset, is the log
    rows = X.witness(fx.st)
    ins = np.concatenate([r[r[:, -1] == 1][:, :16] for r in (rows[6], rows[7])])
    key = lambda a: sorted(map(tuple, np.asarray(a, dtype=np.uint64).tolist()))
    assert key(ins) == key(canon(states))
    with pytest.raises(_lib.RkError):
        p3.verify_hashes(*fx.args)                                   # the unkeyed entry point still refuses prep_width > 0
    assert p3.verify_hashes(*fx.args, prep_root=fx.other_root())[0] == 3 == p3.verify(*fx.args[:3], params=fx.par, prep_root=fx.other_root())


def raw_capture(name, n_arrays, fx, root, sizes):
    """the _key capture `name` called with marker-filled buffers of `sizes` words -> (rc, reported sizes, buffers untouched)"""
    lib = _lib.load()
    arr, keep = p3._c_tables(fx.tables)
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    MARK = 0xA5A5A5A5
    shape = np.full(4, MARK, dtype=np.uint32)
    bufs = [np.full(max(s, 1), MARK, dtype=np.uint32) for s in sizes]
    n = [C.c_size_t(77) for _ in range(n_arrays)]
    rc = getattr(lib, name + "_key")(C.byref(fx.par), arr, len(fx.tables), u(root) if root is not None else None, u(fx.init), fx.init.size,
                                     u(fx.pf), fx.pf.size, u(shape), *[x for b, s in zip(bufs, sizes) for x in (u(b), s)], *[C.byref(v) for v in n])
    del keep
    return rc, [v.value for v in n], all((b == MARK).all() for b in bufs + [shape])


def test_captures_under_another_root_give_the_verdict_and_write_nothing(fx):
    """the verdict is the verifier's.  Under another root that is 3, not 5: the root is the first thing the challenger
    observes behind init, so alpha and zeta move and the constraint identity fails before any opening is looked at
    (csrc/p3_verify.hip: the stages run in order).  Reason 5 is what a changed preprocessed opening gives under the
    right root."""
    spans = RP.parse(fx.full, fx.pf, 1, OVER["queries"])["spans"]
    pf5 = fx.pf.copy()
    at = spans["q4.prep_rows"][0]
    pf5[at] = (int(pf5[at]) + 1) % P
    opened = Fixture(fx.name)
    opened.pf = pf5
    assert p3.verify(fx.tables, pf5, fx.init, params=fx.par, prep_root=fx.root) == 5
    for name, n_arrays in CAPTURES:
        good = T.capture(name, n_arrays, *fx.args, prep_root=fx.root)
        sizes = [a.size for a in good[2:]]
        assert raw_capture(name, n_arrays, fx, fx.root, sizes)[:2] == (0, sizes)
        for word in (0, 7):
            rc, n, untouched = raw_capture(name, n_arrays, fx, fx.other_root(word), sizes)
            assert rc == 3 == p3.verify(*fx.args[:3], params=fx.par, prep_root=fx.other_root(word))
            assert n == [0] * n_arrays and untouched
        rc, n, untouched = raw_capture(name, n_arrays, opened, fx.root, sizes)
        assert rc == 5 and n == [0] * n_arrays and untouched
        # the capacity protocol of the twins: sizes reported, nothing written
        rc, n, untouched = raw_capture(name, n_arrays, fx, fx.root, [0] * n_arrays)
        assert rc == CAPACITY and n == sizes and untouched
        assert T.capture(name, n_arrays, *fx.args, prep_root=fx.other_root())[0] == 3
    for stmt in (F.statement, G.statement, H.statement, X.statement):
        with pytest.raises(_lib.RkError):
            stmt(*fx.args, prep_root=fx.other_root())


def test_root_and_tables_come_together(fx):
    for name, n_arrays in CAPTURES:
        sizes = [1 << 14] * n_arrays
        rc, n, untouched = raw_capture(name, n_arrays, fx, None, sizes)              # preprocessed columns, no root
        assert rc == INVALID and untouched
        with pytest.raises(_lib.RkError) as e:
            T.capture(name, n_arrays, *fx.args)                                      # the unkeyed twin refuses the tables
        assert e.value.status == INVALID
        loose = K.pinned(fx.full)
        for t in loose:
            t.log_height = 0
        with pytest.raises(_lib.RkError) as e:
            T.capture(name, n_arrays, loose, *fx.args[1:], prep_root=fx.root)        # the height of a preprocessed table not pinned
        assert e.value.status == INVALID
    preset, over, _, _ = P3_CASES[UNKEYED_CASE]
    tables, init, blob = tables_of(UNKEYED_CASE), init_of(UNKEYED_CASE), hal.make_params(preset, **over)
    for name, n_arrays in CAPTURES:                                                  # a root, no preprocessed columns: before the proof is read
        with pytest.raises(_lib.RkError) as e:
            T.capture(name, n_arrays, tables, fx.pf, init, blob, prep_root=fx.root)
        assert e.value.status == INVALID
    with pytest.raises(_lib.RkError):
        p3.verify_hashes(tables, fx.pf, init, blob, prep_root=fx.root)


def test_key_captures_with_a_null_root_are_the_unkeyed_ones():
    preset, over, _, _ = P3_CASES[UNKEYED_CASE]
    o.oracle_set_params(preset, **over)
    try:
        tables, init, blob = tables_of(UNKEYED_CASE), init_of(UNKEYED_CASE), hal.make_params(preset, **over)
        pf = o.oracle_p3_prove(tables, init)
        for name, n_arrays in CAPTURES:
            a = T.capture(name, n_arrays, tables, pf, init, blob)
            b = T.capture(name + "_key", n_arrays, tables, pf, init, blob)
            assert a[0] == b[0] == 0 and a[1] == b[1]
            for x, y in zip(a[2:], b[2:]):
                assert x.size and np.array_equal(x, y)
        lib = _lib.load()
        arr, keep = p3._c_tables(tables)
        u = lambda a: a.ctypes.data_as(_lib.u32p)
        rc, states = p3.verify_hashes(tables, pf, init, blob)
        got, n = np.zeros_like(states), C.c_size_t(0)
        assert lib.rk_p3_verify_hashes_key(C.byref(blob), arr, len(tables), None, u(init), init.size, u(pf), pf.size, u(got), got.shape[0],
                                           C.byref(n)) == rc == 0
        assert n.value == states.shape[0] and np.array_equal(got, states)
        del keep
    finally:
        o.oracle_set_params()


# ---------------------------------------------------------------------------------------------- the plans
def test_sizes_accept_the_keyed_layouts(fx):
    st = fx.st
    opn = st.opn
    for sz in (H.sizes(opn), X.sizes(st)):
        assert sz["n_batches"] == len(opn.trees) == (4 if fx.name == "range_prep" else 3)
        assert sz["roots_words"] == 34 == opn.in_roots.size and sz["log_kmax"] == opn.log_kmax and sz["log_pmax"] == opn.log_pmax
        assert sz["ipath_rows"] == st.shape.queries * sum(t.B for t in opn.trees)
        assert sz["paths_words"] == opn.in_paths.size and sz["inputs_words"] == opn.red.in_records.size
        assert sz["n_groups"] == len(opn.groups) and sz["n_slots"] == len(opn.slots)
        assert sz["state_rows"] - sz.get("n_steps", 0) == st.shape.queries * opn.perms_per_query
    assert [t.batch for t in opn.trees] == sorted(t.batch for t in opn.trees) and opn.trees[-1].batch == 3
    assert opn.log_kmax == opn.trees[-1].B and (opn.log_kmax < st.shape.log_max) == (fx.name == "range_prep")
    rsz = G.sizes(st.red)
    assert rsz["n_slots"] == len(st.red.slots) and rsz["inputs_words"] == st.red.in_records.size
    assert tuple(X.sizes(st)[n + "_log_height"] for n in X.TABLE_NAMES) == X.heights(st)
    assert tuple(H.sizes(opn)[n + "_log_height"] for n in H.TABLE_NAMES) == H.heights(opn)
    assert tuple(rsz[n + "_log_height"] for n in G.TABLE_NAMES) == G.heights(st.red)


def test_sizes_refuse_malformed_keyed_layouts(fx):
    lib = _lib.load()
    st = fx.st
    sh, layout = st.shape, list(st.opn.layout)
    u = lambda a: a.ctypes.data_as(_lib.u32p)

    def sizes(lay):
        words = p3.to_mont(np.array(lay, dtype=np.uint64).reshape(-1))
        lead = (sh.log_max, sh.blowup_log2, sh.queries, u(words), len(lay))
        r, op, tr = _lib.RkFriReduceSizeInfo(), _lib.RkFriOpenSizeInfo(), _lib.RkFriTranscriptSizeInfo()
        out = (lib.rk_fri_reduce_sizes(*lead, C.byref(r)), lib.rk_fri_open_sizes(*lead, C.byref(op)),
               lib.rk_fri_transcript_sizes(*lead, u(st.ops_words), len(st.ops), C.byref(tr)))
        assert len(set(out)) == 1
        return out[0]

    assert sizes(layout) == 0
    k = next(i for i, m in enumerate(layout) if m.batch == 3)
    assert k > 0 and layout[k - 1].batch == 0
    swapped = layout[:k - 1] + [layout[k], layout[k - 1]] + layout[k + 1:]               # preprocessed before a trace matrix
    assert sizes(swapped) == INVALID
    assert sizes([layout[0]._replace(batch=3)] + layout[1:]) == INVALID                  # the first matrix is no trace matrix
    assert sizes(layout[:k] + [layout[k]._replace(batch=4)] + layout[k + 1:]) == INVALID
    assert sizes(layout[:k] + [layout[k]._replace(points=1)] + layout[k + 1:]) == INVALID
    tall = layout[k]._replace(log_n=sh.log_max - sh.blowup_log2 + 1, rd=0)               # an LDE taller than log_max
    assert sizes(layout[:k] + [tall] + layout[k + 1:]) == INVALID
    behind = [m for m in layout if m.batch != 3] + [layout[k]]                           # preprocessed behind the quotient
    assert sizes(behind) == INVALID
    # a statement whose roots are the 25-word form while the layout has a fourth batch: the Python side says so
    with pytest.raises(AssertionError):
        H.Statement(st.red, st.opn.in_roots[:25], st.opn.in_paths)


# ---------------------------------------------------------------------------------------------- the statements
def _check_and_prove(fx, mod, st, rows):
    assert [r.shape[0] for r in rows] == [1 << h for h in mod.heights(st)]
    pvs = [canon(v) for v in mod.public_values(st)]
    for air, r, pv in zip(mod.airs(st), rows, pvs):
        assert air.log_quotient_degree() == 1 and air.width == r.shape[1]
        assert air.check_trace(r, pv) == []
    tabs = mod.tables_from_rows(st, rows)
    fp = o.oracle_p3_prove(tabs, st.init)
    assert o.oracle_p3_verify(tabs, fp, st.init) == 0 == p3.verify(tabs, fp, st.init, params=fx.par)      # every bus balanced: no reason 8
    return fp


def test_reduce_statement(fx):
    st = fx.st.red
    fp = _check_and_prove(fx, G, st, G.witness(st))
    assert G.verify_reduce_statement(*fx.args[:3], fp, fx.par, prep_root=fx.root) == 0
    assert G.verify_reduce_statement(*fx.args[:3], fp, fx.par, prep_root=fx.other_root()) == 3
    with pytest.raises(_lib.RkError):
        G.verify_reduce_statement(*fx.args[:3], fp, fx.par)                                              # no root: the tables are refused


def test_open_statement(fx):
    st = fx.st.opn
    rows = H.witness(st)
    fp = _check_and_prove(fx, H, st, rows)
    assert np.array_equal(st.ipath_publics[-8:], fx.root)                                                # the preprocessed tree is last
    assert H.verify_open_statement(*fx.args[:3], fp, fx.par, prep_root=fx.root) == 0
    assert H.verify_open_statement(*fx.args[:3], fp, fx.par, prep_root=fx.other_root()) != 0             # under another root
    red = o.oracle_p3_prove(G.host_tables(st.red), st.red.init)
    assert H.verify_open_statement(*fx.args[:3], red, fx.par, prep_root=fx.root) != 0                    # the smaller statement's proof


def test_transcript_statement(fx):
    st = fx.st
    fp = _check_and_prove(fx, X, st, X.witness(st))
    seg = X.observed_segments(st, fx.init.size, [0] * len(fx.tables))
    assert list(seg)[:3] == ["init", "prep_root", "trace_root"] and seg["prep_root"] == (fx.init.size, 8)
    assert X.verify_transcript_statement(*fx.args[:3], fp, fx.par, prep_root=fx.root) == 0
    assert X.verify_transcript_statement(*fx.args[:3], fp, fx.par, prep_root=fx.other_root()) != 0
    # the binding on the host: a prep_root word changed in `observed` (everything else as captured)
    caps = [F.fri_openings(*fx.args, prep_root=fx.root)[1:], G.fri_inputs(*fx.args, prep_root=fx.root)[1:],
            H.fri_input_paths(*fx.args, prep_root=fx.root)[1:], X.fri_transcript(*fx.args, prep_root=fx.root)[1:]]
    assert X._check_bound(fx.tables, fx.init, fp, fx.par, fx.root, *caps) == 0
    shape, ops, obs, smp = caps[3]
    for word in (0, 7):
        bad = obs.copy()
        at = seg["prep_root"][0] + word
        bad[at] = (int(bad[at]) + 1) % P
        assert X._check_bound(fx.tables, fx.init, fp, fx.par, fx.root, caps[0], caps[1], caps[2], (shape, ops, bad, smp)) == 1
    # ... the roots capture naming another root than the caller's, and a caller without a root
    shape3, roots, paths = caps[2]
    bad = roots.copy()
    bad[25] = (int(bad[25]) + 1) % P
    assert X._check_bound(fx.tables, fx.init, fp, fx.par, fx.root, caps[0], caps[1], (shape3, bad, paths), caps[3]) == 1
    assert X._check_bound(fx.tables, fx.init, fp, fx.par, None, *caps) == 1


# ---------------------------------------------------------------------------------------------- forged statements
def _verdict(fx, mod, st, rows, pubs=None):
    pubs = [canon(v) for v in mod.public_values(st)] if pubs is None else pubs
    tabs = [p3.Table.from_canonical(a, r, pv) for a, r, pv in zip(mod.airs(st), rows, pubs)]
    q = o.oracle_p3_prove(tabs, st.init)
    a, b = o.oracle_p3_verify(tabs, q, st.init), p3.verify(tabs, q, st.init, params=fx.par)
    assert a == b
    return a


def _bad_rows(mod, st, rows, table, pubs=None):
    pubs = [canon(v) for v in mod.public_values(st)] if pubs is None else pubs
    return sorted({r for r, _ in mod.airs(st)[table].check_trace(rows[table], pubs[table])})


def test_forged_preprocessed_openings(rp):
    st = rp.st.opn
    sh = st.shape
    honest = H.witness(st)
    assert _verdict(rp, H, st, honest) == 0
    kt = next(i for i, t in enumerate(st.trees) if t.batch == 3)
    gi = st.trees[kt].top
    g, t = st.groups[gi], st.trees[kt]
    assert g.batch == 3 and kt == len(st.trees) - 1
    rc = G.ReduceCols(len(st.slots))
    OUT, GEND = rc.width + 24, rc.width + 41
    ic = H.IPathCols(len(st.trees))
    rpq = G.rows_per_query(st.slots)
    # an opened preprocessed cell of query 2 changed in the inputs record; reduce'' and the state chip redone from it,
    # ipath and the chip as they were: every table valid in itself, but the digest the sponge sends is no longer the leaf
    # ipath receives -- BUS_IN_LEAF
    q = 2
    rec = p3.from_mont(st.red.in_records).astype(np.uint64).reshape(sh.queries, st.red.per_record).copy()
    at = 1 + st.slots[g.m0].rec_off
    assert st.layout[st.slots[g.m0].matrix].batch == 3
    rec[q, at] = (int(rec[q, at]) + 1) % P
    redone = H.witness(st, records=rec)
    rows = [honest[0], honest[1], redone[2], honest[3], honest[4], redone[5]]
    end = q * rpq + g.row0 + g.cells - 1
    first = t.row0 + q * t.B
    assert rows[2][end][GEND] == 1 and rows[3][first][ic.FIRST] == 1 and rows[3][first][ic.BATCH] == 3
    assert np.array_equal(honest[2][end][OUT: OUT + 8], honest[3][first][ic.CUR: ic.CUR + 8])
    assert not np.array_equal(rows[2][end][OUT: OUT + 8], rows[3][first][ic.CUR: ic.CUR + 8])
    assert [_bad_rows(H, st, rows, i) for i in range(6)] == [[]] * 6
    assert _verdict(rp, H, st, rows) == 8
    # ... and with ipath and the chip redone too: the path of that query's preprocessed tree no longer reaches the root,
    # the constraint on its last row and nothing else
    assert [_bad_rows(H, st, redone, i) for i in (0, 1, 2, 4, 5)] == [[]] * 5
    assert _bad_rows(H, st, redone, 3) == [first + t.B - 1]
    # the preprocessed root among the public values changed: the root constraint of ipath
    for word in (0, 7):
        pubs = [canon(v) for v in H.public_values(st)]
        assert pubs[3].size == 8 * len(st.trees)
        pubs[3][8 * kt + word] = (int(pubs[3][8 * kt + word]) + 1) % P
        assert _bad_rows(H, st, honest, 3, pubs) == [t.row0 + qq * t.B + t.B - 1 for qq in range(sh.queries)]
        assert _verdict(rp, H, st, honest, pubs) == 3


def test_forged_observed_root(rp):
    """the root the chain observes is a public value of the transcript table: another word there and the row that
    absorbs it breaks IN = observed"""
    st = rp.st
    rows = X.witness(st)
    seg = X.observed_segments(st, rp.init.size, [0] * len(rp.tables))
    pubs = [canon(v) for v in X.public_values(st)]
    at = seg["prep_root"][0] + 2
    pubs[4][at] = (int(pubs[4][at]) + 1) % P
    step = next(i for i, s in enumerate(st.plan.steps) if s.obs_off <= at < s.obs_off + s.n_in)
    assert _bad_rows(X, st, rows, 4, pubs) == [step]
    assert _verdict(rp, X, st, rows, pubs) == 3


# ---------------------------------------------------------------------------------------------- the lane bodies on the CPU
def test_kernel_lanes_on_the_cpu(fx, tmp_path):
    """no lane body of p3_kernels.hpp changed for the fourth batch; the plan that feeds them did.  The open lanes (sponge,
    fill, ipath) walked on the CPU over the keyed plan -- batch 3 in the flags, four levels, the preprocessed path last
    in a record -- against the numpy witness"""
    so = str(tmp_path / "libemul_fri_open.so")
    src = os.path.join(o.EMUL_DIR, "emul_fri_open.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(o.ROOT, "raiko_amd", "csrc"), "-o", so, src],
                   check=True, capture_output=True)
    lib = C.CDLL(so)
    st = fx.st.opn
    want = [p3.to_mont(r) for r in H.witness(st)]
    rc_ext, rc_int, diag, m4 = R.tables_of()
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
    assert 3 in groups.reshape(-1, 8)[:, 5] and levels.reshape(-1, 40)[-1, 0] == 3
    slots = np.array([[s.rd, s.width, s.points, s.rec_off, 0, int(s.last_of_round), s.row0, 0] for s in st.slots], dtype=np.uint32).reshape(-1)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.emul_fri_open_rows(sh.log_max, sh.queries, len(st.slots), len(st.groups), len(st.trees), G.rows_per_query(st.slots), reduce.shape[1],
                           C.c_size_t(st.red.per_record), C.c_size_t(st.per_path), C.c_size_t(n0), vp(slots), vp(groups), vp(rowinfo), vp(levels),
                           vp(st.red.in_records), vp(st.in_paths), vp(tab), m4, vp(reduce), vp(ipath), vp(chip_in), vp(chip_mult), vp(chip),
                           C.c_size_t(chip.shape[0]), vp(state), C.c_size_t(state.shape[0]))
    for g_, w in zip((reduce, ipath, chip, state), want[2:]):
        assert np.array_equal(g_, w), np.argwhere(g_ != w)[:8]
