"""Preprocessed columns without a GPU: the AIR front end (rk_air_create_prep), the proof-size formula, the permutation
lane body over preprocessed columns (tests/emul), and the host verifier rk_p3_verify_key on the committed fixtures of
tests/golden/p3-prep (made on the GPU by tools/make_p3_prep_golden.py), which the exact reference of
tests/p3_ref_prep.py accepts too."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as o
import p3_prep_cases as K
import p3_ref as R
import p3_ref_prep as RP
from raiko_amd import _lib, hal as H, p3

P = p3.P
GOLDEN = os.path.join(o.ROOT, "tests", "golden", "p3-prep")
OVER = dict(queries=7, pow_bits=2)        # tools/make_p3_prep_golden.py
INVALID = _lib.RK_ERR_INVALID


def _create(steps, width, prep_width, ix=(), n_ix=0, ext_w=0, n_public=0):
    lib = _lib.load()
    st = np.ascontiguousarray(steps, dtype=np.uint32).reshape(-1, 3)
    iw = np.ascontiguousarray(ix, dtype=np.uint32)
    h = C.c_void_p()
    rc = lib.rk_air_create_prep(st.ctypes.data if st.size else None, st.shape[0], width, prep_width, n_public,
                                iw.ctypes.data_as(_lib.u32p) if iw.size else None, n_ix, iw.size, ext_w, C.byref(h))
    return rc, h


def test_air_create_prep_validation():
    lib = _lib.load()
    ok = [(p3.PREP_LOCAL, 1, 0), (p3.PREP_NEXT, 0, 0), (p3.SUB, 0, 1), (p3.ASSERT_ZERO, 2, 0)]
    rc, h = _create(ok, 1, 2)
    assert rc == 0 and lib.rk_air_prep_width(h) == 2
    n = C.c_size_t(0)
    assert lib.rk_air_get_steps(h, None, 0, C.byref(n)) == _lib.RK_ERR_CAPACITY and n.value == 4
    back = np.zeros((4, 3), dtype=np.uint32)
    assert lib.rk_air_get_steps(h, back.ctypes.data, 4, C.byref(n)) == 0 and back.tolist() == [list(s) for s in ok]   # round trip
    lib.rk_air_destroy(h)
    for op in (p3.PREP_LOCAL, p3.PREP_NEXT):               # operand >= prep_width
        assert _create([(op, 2, 0), (p3.ASSERT_ZERO, 0, 0)], 1, 2)[0] == INVALID
        assert _create([(op, 0, 0), (p3.ASSERT_ZERO, 0, 0)], 1, 0)[0] == INVALID
    # the existing constructors refuse PREP_* ops
    st = np.array([(p3.PREP_LOCAL, 0, 0), (p3.ASSERT_ZERO, 0, 0)], dtype=np.uint32)
    h = C.c_void_p()
    assert lib.rk_air_create(st.ctypes.data, 2, 3, 0, C.byref(h)) == INVALID
    ix = np.array([1, 1, 0, 0, 1, 0], dtype=np.uint32)
    assert lib.rk_air_create_lookup(st.ctypes.data, 2, 3, 0, ix.ctypes.data_as(_lib.u32p), 1, ix.size, 0, C.byref(h)) == INVALID
    assert lib.rk_air_prep_width(None) == 0
    # interactions over the union: column width + prep_width - 1 is the last one, width + prep_width is refused, as a
    # value and as a mult that is a column
    own = [(p3.LOCAL, 0, 0), (p3.ASSERT_ZERO, 0, 0)]
    rc, h = _create(own, 2, 3, [1, 1, 0, 4, 2, 0, 4], 1, ext_w=11)
    assert rc == 0
    full = np.zeros((4096, 3), dtype=np.uint32)
    assert lib.rk_air_get_steps(h, full.ctypes.data, 4096, C.byref(n)) == 0
    full = full[: n.value]
    assert (p3.PREP_LOCAL, 2) in {(int(a), int(b)) for a, b, _ in full}          # the appended constraints read it through PREP_LOCAL
    assert not any(int(a) == p3.LOCAL and int(b) >= 2 for a, b, _ in full)
    lib.rk_air_destroy(h)
    assert _create(own, 2, 3, [1, 1, 0, 4, 2, 0, 5], 1, ext_w=11)[0] == INVALID
    assert _create(own, 2, 3, [1, 1, 0, 5, 2, 0, 4], 1, ext_w=11)[0] == INVALID
    assert _create(own, 2, 0, [1, 1, 0, 1, 1, 2], 1, ext_w=11)[0] == INVALID
    # n_interactions = 0: an AIR without lookups; the library's list and AirBuilder's are the same identities
    b = p3.AirBuilder(2, 0, prep_width=3)
    b.assert_zero(b.local(0))
    b.receive(1, [0, b.prep(2)], mult=b.prep(2), mult_is_const=False)
    mine, theirs = b.build(), None
    b2 = p3.AirBuilder(2, 0, prep_width=3)
    b2.assert_zero(b2.local(0))
    b2.receive(1, [0, b2.prep(2)], mult=b2.prep(2), mult_is_const=False)
    theirs = b2.build(library_constraints=True)
    assert theirs.prep_width == 3 and theirs.n_constraints == mine.n_constraints and theirs.info()["max_degree"] == mine.info()["max_degree"]


def test_quotient_degree_through_a_preprocessed_column():
    """prep . local . local has symbolic degree 3: log2_ceil(3 - 1) = 1, two chunks; prep . local degree 2: one"""
    b = p3.AirBuilder(2, 0, prep_width=1)
    b.assert_zero(b.prep_local(0) * b.local(0) * b.local(1))
    air = b.build()
    assert air.info()["max_degree"] == 3 and air.info()["log_quotient_degree"] == 1 == air.log_quotient_degree()
    b = p3.AirBuilder(2, 0, prep_width=1)
    b.assert_zero(b.prep_next(0) * b.local(0) - b.local(1))
    air = b.build()
    assert air.info()["max_degree"] == 2 and air.info()["log_quotient_degree"] == 0 == air.log_quotient_degree()
    assert K.gate_air(5, True).info()["log_quotient_degree"] == 1 and K.gate_air(1).info()["log_quotient_degree"] == 0


def _shapes():
    fib = lambda k: p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(k))
    yield [K.gate_table(1, 1)]
    yield [K.gate_table(3, 5, True)]
    yield [K.gate_table(6, 5, True)]
    yield [fib(4), K.gate_table(3, 5, True), p3.Table.from_canonical(p3.cubic_air(6), *p3.cubic_trace(5, 6, seed=2))]
    yield [fib(6), K.gate_table(3, 1)]
    yield [fib(2), K.gate_table(6, 5)]
    yield K.mix_tables(6)
    yield p3.lookup_demo_tables_prep(4, 4)
    yield p3.lookup_demo_tables_prep(10, 4)


def test_proof_size_formula():
    """p3h::Layout through rk_p3_proof_bound_words_key against the reference parser's count, for the shapes the GPU tests
    prove; without preprocessed columns it is rk_p3_proof_bound_words, which is 0 for tables that have them"""
    lib = _lib.load()
    for queries, blow in ((3, 1), (7, 2)):
        par = H.make_params(1, queries=queries, pow_bits=1, blowup_log2=blow)
        for tables in _shapes():
            arr, keep = p3._c_tables(tables)
            assert lib.rk_p3_proof_bound_words_key(C.byref(par), arr, len(tables)) == RP.proof_words(tables, blow, queries)
            assert lib.rk_p3_proof_bound_words(C.byref(par), arr, len(tables)) == 0
        for tables in ([p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(5))], p3.lookup_demo_tables(5, 3, seed=1)):
            arr, keep = p3._c_tables(tables)
            want = lib.rk_p3_proof_bound_words(C.byref(par), arr, len(tables))
            assert want and lib.rk_p3_proof_bound_words_key(C.byref(par), arr, len(tables)) == want == RP.proof_words(tables, blow, queries)


@pytest.mark.parametrize("n", [2, 256, 300, 513])
def test_permutation_lanes_over_preprocessed_columns(tmp_path, n):
    """p3k::perm_stage / perm_row with a preprocessed matrix beside the trace, every row against the numpy restatement:
    tuples mixing main and preprocessed columns, a tuple of preprocessed columns only, multiplicities from a preprocessed
    column and from a main one; a partial workgroup, exactly one, and the rows of a partial last one"""
    so = str(tmp_path / "libemul_p3_prep.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(o.ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(o.EMUL_DIR, "emul_p3_prep.cpp")], check=True, capture_output=True)
    lib = C.CDLL(so)
    w, cw = 4, 70
    g = np.random.default_rng(n)
    trace = g.integers(0, P, size=(n, w)).astype(np.uint64)
    prep = g.integers(0, P, size=(n, cw)).astype(np.uint64)
    prep[:, 1] = g.integers(0, 3, size=n)
    prep[0, 1], prep[n - 1, 1] = P - 1, 0
    its = [p3.Interaction(p3.SEND, 3, [0, w + 0, 2, w + 69], w + 1), p3.Interaction(p3.RECEIVE, P - 1, [w + 5, w + 6], 3),
           p3.Interaction(p3.SEND, 7, list(range(w + 2, w + 66)), 2, True)]
    chal = R.challenge_words(((3, P - 1, 0, 9), (P - 5, 2, 77, 1)), 11, 64)
    used, flat = [], []
    slot = lambda c: used.index(c) if c in used else (used.append(c) or len(used) - 1)
    mont = lambda v: int(p3.to_mont([v])[0])
    for it in its:
        flat += [it.kind, mont(it.bus), int(it.mult_is_const), mont(it.mult) if it.mult_is_const else slot(it.mult), len(it.value_cols)]
        flat += [slot(c) for c in it.value_cols]
    assert 64 < len(used) <= 120
    desc = np.concatenate([p3.to_mont(chal), np.array(flat, dtype=np.uint32), np.array(used, dtype=np.uint32)]).astype(np.uint32)
    got = np.full((4 * 3, n), 0xFFFFFFFF, dtype=np.uint32)
    tm, pm = np.ascontiguousarray(p3.to_mont(trace)), np.ascontiguousarray(p3.to_mont(prep))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.emul_perm_entries_prep(vp(got), vp(tm), vp(pm), vp(desc), C.c_size_t(n), C.c_size_t(w), C.c_size_t(cw), len(chal), len(its), mont(11),
                               len(used), len(chal) + len(flat))
    entries, totals = RP.perm_entries(trace, prep, its, chal, 11)
    want = np.concatenate([entries.reshape(n, 8), totals], axis=1)
    assert int(got.max()) < P
    bad = np.argwhere(p3.from_mont(got).T.astype(np.uint64) != want)
    assert bad.size == 0, "first differing (row, column): %s" % bad[:4].tolist()


# ---------------------------------------------------------------- the fixtures
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    if name == "range_prep":
        cpu, add, mul, _ = p3.lookup_demo_airs()
        airs = [cpu, add, mul, p3.p3_range_air_prep()]
    else:
        airs = [K.gate_air(2, True)]
    tables = [p3.Table(a, z["trace%d" % i], (), prep=z["prep%d" % i] if "prep%d" % i in z.files else None) for i, a in enumerate(airs)]
    return tables, z["proof"], z["root"], z["init"]


@pytest.fixture(scope="module", params=["range_prep", "gate_next"])
def fx(request):
    tables, pf, root, init = _fixture(request.param)
    return tables, pf, root, init, H.make_params(1, **OVER)


def test_fixture_is_accepted_by_verifier_and_reference(fx):
    tables, pf, root, init, par = fx
    ver = K.pinned(tables)
    assert p3.verify(ver, pf, init, params=par, prep_root=root) == 0
    assert p3.verify(tables, pf, init, params=par, prep_root=root) == 0           # heights from full tables pin the same
    R.p2_tables(1)
    RP.check_proof(1, 1, tables, init, pf, root, queries=OVER["queries"])
    assert pf.size < 8000


def test_fixture_refused_under_another_key(fx):
    tables, pf, root, init, par = fx
    ver = K.pinned(tables)
    for i in (0, 7):
        bad = root.copy()
        bad[i] = (int(bad[i]) + 1) % P
        assert p3.verify(ver, pf, init, params=par, prep_root=bad) != 0          # one root word changed
    ti = next(i for i, t in enumerate(tables) if t.air.prep_width)
    taller = K.pinned(tables)
    taller[ti].log_height += 1
    assert p3.verify(taller, pf, init, params=par, prep_root=root) == 2          # the pinned height changed
    loose = K.pinned(tables)
    loose[ti].log_height = 0
    assert p3.verify(loose, pf, init, params=par, prep_root=root) == INVALID     # the height left unpinned
    assert p3.verify(ver, pf, init, params=par) == INVALID                       # rk_p3_verify does not know the batch
    lib = _lib.load()
    arr, keep = p3._c_tables(ver)
    iw, pw = init.ctypes.data_as(_lib.u32p), pf.ctypes.data_as(_lib.u32p)
    assert lib.rk_p3_verify_key(C.byref(par), arr, len(ver), None, iw, init.size, pw, pf.size) == INVALID    # tables with prep, no root
    plain = [p3.Table(p3.fibonacci_air(), None, p3.to_mont([0, 1, 5]))]
    parr, pkeep = p3._c_tables(plain)
    assert lib.rk_p3_verify_key(C.byref(par), parr, 1, root.ctypes.data_as(_lib.u32p), iw, init.size, pw, pf.size) == INVALID   # a root, no prep


def test_fixture_single_word_mutations_of_the_preprocessed_parts(fx):
    """every word of the preprocessed opened values (constraint identity or, the opened value being bound by the reduced
    openings, a later stage: never 0), and every word of the preprocessed rows and paths of the queries (reason 5: the
    opening no longer leads to the caller's root)"""
    tables, pf, root, init, par = fx
    ver = K.pinned(tables)
    spans = RP.parse(tables, pf, 1, OVER["queries"])["spans"]
    head = [w for name, (a, b) in spans.items() if name.startswith("head.") for w in range(a, b)]
    query = [w for name, (a, b) in spans.items() if name.endswith((".prep_rows", ".prep_path")) for w in range(a, b)]
    assert head and len(query) >= OVER["queries"] * 9
    for at in head:
        m = pf.copy()
        m[at] = (int(m[at]) + 1) % P
        assert p3.verify(ver, m, init, params=par, prep_root=root) in (3, 6, 7), at
    for at in query:
        m = pf.copy()
        m[at] = (int(m[at]) + 1) % P
        assert p3.verify(ver, m, init, params=par, prep_root=root) == 5, at


def test_other_entry_points_refuse_preprocessed_tables(fx):
    tables, pf, root, init, par = fx
    lib = _lib.load()
    ver = K.pinned(tables)
    arr, keep = p3._c_tables(ver)
    nt = len(ver)
    with pytest.raises(_lib.RkError) as e:
        p3.verify_hashes(ver, pf, init, params=par)
    assert e.value.status == INVALID
    shape, w = (C.c_uint32 * 4)(), [C.c_size_t(0) for _ in range(3)]
    buf = np.zeros(1 << 18, dtype=np.uint32)
    bp, cap, ip, pw = buf.ctypes.data_as(_lib.u32p), buf.size, init.ctypes.data_as(_lib.u32p), pf.ctypes.data_as(_lib.u32p)
    r = [C.byref(x) for x in w]
    assert lib.rk_p3_fri_openings(C.byref(par), arr, nt, ip, init.size, pw, pf.size, shape, bp, cap, bp, cap, r[0], r[1]) == INVALID
    assert lib.rk_p3_fri_inputs(C.byref(par), arr, nt, ip, init.size, pw, pf.size, shape, bp, cap, bp, cap, bp, cap, r[0], r[1], r[2]) == INVALID
    assert lib.rk_p3_fri_input_paths(C.byref(par), arr, nt, ip, init.size, pw, pf.size, shape, bp, cap, bp, cap, r[0], r[1]) == INVALID
    assert lib.rk_p3_fri_transcript(C.byref(par), arr, nt, ip, init.size, pw, pf.size, shape, bp, cap, bp, cap, bp, cap, r[0], r[1], r[2]) == INVALID
    # a shard carries no key: refused before a device is looked for
    parr, pkeep = p3._c_tables(tables)
    sh = (_lib.RkP3Shard * 1)()
    sh[0].tables, sh[0].n_tables = parr, nt
    sh[0].init_words, sh[0].n_init = ip, init.size
    sh[0].h_proof, sh[0].capacity_words = bp, cap
    opts = _lib.RkP3SessionOpts(device=0, batch=1, verify=0, params=C.pointer(par))
    failed = C.c_size_t(99)
    assert lib.rk_p3_prove_shards(C.byref(opts), sh, 1, C.byref(failed)) == INVALID and failed.value == 0
