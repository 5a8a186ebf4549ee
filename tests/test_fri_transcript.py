"""The Fiat-Shamir transcript of the FRI query check as lookup tables (raiko_amd/fri_transcript.py, rk_p3_fri_transcript): the
CPU side, through the oracle as tests/test_fri_open.py.  The plan is replayed in plain Python from the captured calls and
gives the captured samples; the numpy witness satisfies all eight AIRs, the oracle proves them and both verifiers accept;
the lane bodies of the GPU kernels write the witness word for word on the CPU.  What the statement adds: the tables of a
shard proof made under another `init` are refused when the transcript's public values claim this one.  Forged witnesses
are refused with reason 3 (a constraint) or 8 (a bus; the verifier checks the cumulative sums first)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import field_ref as FR
import fri_param_sets as PS
import oracle_lib as o
import p2_chip_ref as R
from p3_cases import P3_CASES, tables_of
from raiko_amd import _lib, hal, p3
from raiko_amd import fri_chip as F
from raiko_amd import fri_open as H
from raiko_amd import fri_reduce as G
from raiko_amd import fri_transcript as X
import test_gpu_fri_open
from test_gpu_fri_transcript import ROW_CASES as FULL

P = o.P
QUERIES = (7, 8, 100)
# FULL: the cases of tests/test_gpu_fri_open.py, the statement built in full for each once: (queries, init, further overrides)
ROW_CASES = list(FULL)
FORGE = ("sp1_lookup_beside_plain",) + FULL["sp1_lookup_beside_plain"]
assert sorted(FULL) == sorted(test_gpu_fri_open.ROW_CASES)


@pytest.fixture()
def params():
    yield o.oracle_set_params
    o.oracle_set_params()


_SHARDS = {}


def setup(params, case, queries, init, more=()):
    """the case's shard proof under `queries` and `init`, made once and shared (nothing changes it)"""
    preset, over, _, _ = P3_CASES[case]
    over = dict(over, queries=queries, **dict(more))
    params(preset, **over)
    blob = hal.make_params(preset, **over)
    key = (case, queries, tuple(init), tuple(sorted(dict(more).items())))
    if key not in _SHARDS:
        tables, iw = tables_of(case), p3.to_mont(np.array(init, dtype=np.uint64))
        _SHARDS[key] = (tables, iw, o.oracle_p3_prove(tables, iw))
    return (blob,) + _SHARDS[key]


def challenger_replay(ops, observed, consts):
    """csrc/p3_host.hpp's DuplexChallenger in plain Python over canonical words -> (sampled, absorbed words per duplex)"""
    state, buf, out, at, sampled, duplexes = [0] * 16, [], [], 0, [], []

    def duplex():
        nonlocal state, buf, out
        state[: len(buf)] = buf
        duplexes.append(len(buf))
        buf = []
        state = [int(v) for v in H._permute16(np.array([state], dtype=np.uint64), consts)[0]]
        out = state[:8]

    for kind, count in ops:
        if kind == X.OBSERVE:
            for _ in range(count):
                out = []
                buf.append(int(observed[at]))
                at += 1
                if len(buf) == 8:
                    duplex()
        else:
            for _ in range(count if kind == X.SAMPLE else 1):
                if buf or not out:
                    duplex()
                sampled.append(out.pop())
    assert at == len(observed)
    return sampled, duplexes


@pytest.mark.parametrize("case", ROW_CASES)
def test_plan_against_the_capture(params, case):
    """the plan -- which step absorbs what, which cell every sample pops -- replayed from `ops` alone gives `sampled`"""
    init = FULL[case][1]
    for queries in QUERIES:
        blob, tables, iw, pf = setup(params, case, queries, init)
        rc, shape, ops, obs, smp = X.fri_transcript(tables, pf, iw, blob)
        assert rc == 0 == p3.verify(tables, pf, iw, params=blob) and shape.queries == queries
        ops_c = [tuple(int(v) for v in p) for p in p3.from_mont(ops).reshape(-1, 2)]
        consts = F.poseidon2_tables(blob)
        sampled, duplexes = challenger_replay(ops_c, p3.from_mont(obs), consts)
        assert sampled == [int(v) for v in p3.from_mont(smp)]
        plan = X.plan_of(ops_c, shape.log_max)
        assert [s.n_in for s in plan.steps] == duplexes and plan.n_obs == obs.size and plan.n_pub + plan.n_bits == smp.size
        assert plan.n_bits == queries + 1 and plan.pow_bits == int(blob.pow_bits) and len(plan.steps) < 100
        # what the verifier observed first and last, and the indices the query check used
        nt = int(pf[0])
        assert np.array_equal(obs[: iw.size], iw) and np.array_equal(obs[iw.size: iw.size + 8], pf[1 + nt: 9 + nt])
        rc, _, _, rec = F.fri_openings(tables, pf, iw, blob)
        idx = p3.from_mont(rec.reshape(queries, -1)[:, 0])
        tail = p3.from_mont(smp[plan.n_pub:])
        assert np.array_equal(tail[1:] & np.uint32((1 << shape.log_max) - 1), idx) and int(tail[0]) & ((1 << plan.pow_bits) - 1) == 0


def plan_for(params, case, queries, init, more):
    blob, tables, iw, pf = setup(params, case, queries, init, more)
    rc, shape, ops, obs, smp = X.fri_transcript(tables, pf, iw, blob)
    assert rc == 0
    n_perm = sum(t.air.perm_width > 0 for t in tables)
    return X.plan_of([tuple(int(v) for v in p) for p in p3.from_mont(ops).reshape(-1, 2)], shape.log_max), n_perm


def test_cases_exhibit_every_class(params):
    seen = set()
    for case, (queries, init, more) in FULL.items():
        plan, n_perm = plan_for(params, case, queries, init, more)
        st = plan.steps
        for i, s in enumerate(st):
            pops = bool(s.pub or s.bits)
            if s.n_in == 8 and pops:
                seen.add("the eighth word fires the duplex and the sample takes no second one")
            if 0 < s.n_in < 8:
                assert pops
                seen.add("a sample fires the duplex over a partial buffer")
            if s.n_in == 0:
                assert queries >= 8 and pops
                seen.add("a duplex that absorbs nothing")
        if queries == 7:
            assert sorted(st[-1].bits.items()) == [(7 - k, k) for k in range(7, -1, -1)] and st[-1].n_in > 0
            seen.add("the indices end with the proof-of-work block")
        else:
            assert all(s.n_in == 0 and not s.pub for s in st[-((queries - 7 + 7) // 8):])
        seen.add("a permutation batch" if n_perm else "no permutation batch")
        seen.add("an init" if init else "an empty init")
        if plan.pow_bits == 0:
            seen.add("pow_bits = 0")
    assert seen == {"the eighth word fires the duplex and the sample takes no second one", "a sample fires the duplex over a partial buffer",
                    "a duplex that absorbs nothing", "the indices end with the proof-of-work block", "a permutation batch",
                    "no permutation batch", "an init", "an empty init", "pow_bits = 0"}


@pytest.mark.parametrize("case", ROW_CASES)
def test_honest_statement(params, case):
    queries, init, more = FULL[case]
    blob, tables, iw, pf = setup(params, case, queries, init, more)
    st = X.statement(tables, pf, iw, blob)
    rows = X.witness(st)
    assert [r.shape[0] for r in rows] == [1 << h for h in X.heights(st)]
    sz = X.sizes(st)
    assert tuple(sz[n + "_log_height"] for n in X.TABLE_NAMES) == X.heights(st)
    assert [sz[n + "_width"] for n in X.TABLE_NAMES] == [r.shape[1] for r in rows]
    assert (sz["n_steps"], sz["pow_bits"], sz["observed_words"]) == (len(st.plan.steps), st.plan.pow_bits, st.observed.size)
    assert sz["transcript_publics_words"] == st.transcript_publics.size and sz["bits_rows"] == queries + 1
    assert int(rows[7][:, -1].sum()) == sz["state_rows"] == H.sizes(st.opn)["state_rows"] + sz["n_steps"]
    pvs = [FR.from_mont(v.astype(np.uint64)) for v in X.public_values(st)]
    for t, (air, r, pv) in enumerate(zip(X.airs(st), rows, pvs)):
        assert air.log_quotient_degree() == 1 and air.width == r.shape[1]
        # row by row in Python; at 100 queries only the tables this statement adds or changes (the proof below, which both
        # verifiers accept, stands for the constraints of all eight)
        if queries < 100 or t in (0, 4, 5):
            assert air.check_trace(r, pv) == []
    for t in (4, 5):                       # every multiplicity column is 0 on padding rows
        n_real = len(st.plan.steps) if t == 4 else queries + 1
        assert not rows[t][n_real:].any()
    tabs = X.tables_from_rows(st, rows)
    fp = o.oracle_p3_prove(tabs, st.init)
    assert o.oracle_p3_verify(tabs, fp, st.init) == 0 == p3.verify(tabs, fp, st.init, params=blob)
    assert X.verify_transcript_statement(tables, pf, iw, fp, blob) == 0
    if case == ROW_CASES[0]:
        # the proof of the smaller statement is no proof of this one; another init is another transcript
        opn = o.oracle_p3_prove(H.host_tables(st.opn), st.opn.init)
        assert X.verify_transcript_statement(tables, pf, iw, opn, blob) != 0
        other = iw.copy()
        other[0] = p3.to_mont([1])[0]
        assert p3.verify(tables, pf, other, params=blob) != 0 != X.verify_transcript_statement(tables, pf, other, fp, blob)


@pytest.mark.parametrize("pset,case", PS.ROW_IDS, ids=[PS.row_id(*x) for x in PS.ROW_IDS])
def test_reference_holds_under_parameter_sets(params, pset, case):
    """the oracle and the numpy witness alone under every set of tests/fri_param_sets.py; the challenger replayed in plain
    Python under the set's constants and matrix gives the captured samples"""
    st, rows = PS.check_reference(X, X.verify_transcript_statement, pset, case, transcript=True)
    blob, tables, iw, pf = PS.cpu_shard(pset, case, transcript=True)
    sz = X.sizes(st)
    assert [r.shape[0] for r in rows] == [1 << h for h in X.heights(st)]
    assert int(rows[7][:, -1].sum()) == sz["state_rows"] == H.sizes(st.opn)["state_rows"] + sz["n_steps"]
    assert st.plan.pow_bits == int(blob.pow_bits) >= 1 and st.shape.queries == PS.TRANSCRIPT_SHARDS[case][0]
    rc, shape, ops, obs, smp = X.fri_transcript(tables, pf, iw, blob)
    ops_c = [tuple(int(v) for v in p) for p in p3.from_mont(ops).reshape(-1, 2)]
    consts = F.poseidon2_tables(blob)
    assert consts[3] == int(blob.p2_m4)
    sampled, _ = challenger_replay(ops_c, p3.from_mont(obs), consts)
    assert rc == 0 and sampled == [int(v) for v in p3.from_mont(smp)]


def test_fold_air_without_the_index_bus_is_unchanged(params):
    sh = F.Shape(9, 8, 1, 10)
    a, b_ = F.fri_fold_air(sh, coset_shift=31), F.fri_fold_air(sh, coset_shift=31, index_bus=False)
    assert np.array_equal(a.steps, b_.steps) and len(a.interactions) == 3
    c = F.fri_fold_air(sh, coset_shift=31, index_bus=True)
    assert c.width == a.width + 1 and len(c.interactions) == 4 and c.log_quotient_degree() == 1
    assert [i.value_cols for i in c.interactions[:3]] == [i.value_cols for i in a.interactions]
    assert (c.interactions[3].bus, c.interactions[3].mult) == (F.BUS_FRI_INDEX, a.width)


def test_new_entry_points_refuse_malformed_arguments(params):
    queries, init, more = FULL[ROW_CASES[0]]
    blob, tables, iw, pf = setup(params, ROW_CASES[0], queries, init, more)
    lib = _lib.load()
    arr, keep = p3._c_tables(tables)
    n = [C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)]
    shape = np.zeros(4, dtype=np.uint32)
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    call = lambda par, sh, a, b, c: lib.rk_p3_fri_transcript(par, arr, len(tables), u(iw), iw.size, u(pf), pf.size, sh, None, 0, None, 0, None, 0, a, b, c)
    refs = [C.byref(v) for v in n]
    assert call(C.byref(blob), None, *refs) == -1
    for k in range(3):
        assert call(C.byref(blob), u(shape), *[None if j == k else r for j, r in enumerate(refs)]) == -1
    assert call(C.byref(blob), u(shape), *refs) == _lib.RK_ERR_CAPACITY and not shape.any()
    st = X.statement(tables, pf, iw, blob)
    assert [v.value for v in n] == [st.ops_words.size, st.observed.size, st.sampled.size]
    bad_pf = pf.copy()
    bad_pf[-1] = (int(bad_pf[-1]) + 1) % P
    assert lib.rk_p3_fri_transcript(C.byref(blob), arr, len(tables), u(iw), iw.size, u(bad_pf), pf.size, u(shape), None, 0, None, 0, None, 0, *refs) > 0
    assert [v.value for v in n] == [0, 0, 0] and not shape.any()
    for bad in (hal.make_params(0, queries=10), hal.make_params(1, queries=10, pow_bits=7, fri_fold_log2=4),
                hal.make_params(1, queries=10, pow_bits=7, p2_pad_free=0)):
        assert call(C.byref(bad), u(shape), *refs) == -1
        with pytest.raises(_lib.RkError):
            X.statement(tables, pf, iw, bad)
        with pytest.raises(_lib.RkError):
            X.verify_transcript_statement(tables, pf, iw, pf, bad)
    del keep
    sh, lw, ow = st.shape, st.opn.layout_words, st.ops_words
    out = _lib.RkFriTranscriptSizeInfo()
    sizes = lambda q, ops, n_ops: lib.rk_fri_transcript_sizes(sh.log_max, sh.blowup_log2, q, u(lw), len(st.opn.layout), u(ops) if ops is not None else None,
                                                              n_ops, C.byref(out))
    assert sizes(sh.queries, ow, len(st.ops)) == 0
    assert sizes(sh.queries, None, len(st.ops)) == -1 and sizes(sh.queries, ow, 0) == -1
    assert sizes(sh.queries + 1, ow, len(st.ops)) == -1 and sizes(sh.queries, ow, len(st.ops) - 1) == -1     # not queries + 1 sample_bits
    assert lib.rk_fri_transcript_sizes(sh.log_max, sh.blowup_log2, sh.queries, u(lw), len(st.opn.layout), u(ow), len(st.ops), None) == -1
    swapped = ow.copy()
    swapped[-2:], swapped[-4:-2] = p3.to_mont([X.OBSERVE, 1]), ow[-2:]                  # an observe behind a sample_bits
    assert sizes(sh.queries, swapped, len(st.ops)) == -1
    wrong_bits = ow.copy()
    wrong_bits[-1] = p3.to_mont([sh.log_max - 1])[0]                                     # an index of another length
    assert sizes(sh.queries, wrong_bits, len(st.ops)) == -1
    assert lib.rk_fri_transcript_rows_device(None, sh.log_max, sh.blowup_log2, sh.queries, u(lw), len(st.opn.layout), u(ow), len(st.ops),
                                             *([None] * 7), *([None, 0] * 8)) == -1


# ---------------------------------------------------------------------------------------------- what the statement adds; forgeries
class Forge:
    def __init__(self, pset=None):
        case, queries, init, more = FORGE
        if pset is None:
            self.blob, self.tables, self.iw, self.pf = setup(o.oracle_set_params, case, queries, init, more)
        else:
            self.blob, self.tables, self.iw, self.pf = PS.cpu_shard(pset, case, transcript=True)
        self.st = X.statement(self.tables, self.pf, self.iw, self.blob)
        self.rows = X.witness(self.st)
        self.pubs = [FR.from_mont(v.astype(np.uint64)) for v in X.public_values(self.st)]
        self.tc, self.bc = X.TranscriptCols(len(self.st.plan.steps)), X.BitsCols

    def copy(self):
        return [r.copy() for r in self.rows]

    def bad_rows(self, rows, table, pubs=None, st=None):
        pubs = self.pubs if pubs is None else pubs
        return sorted({r for r, _ in X.airs(st or self.st)[table].check_trace(rows[table], pubs[table])})

    def verdict(self, rows, pubs=None, st=None):
        pubs = self.pubs if pubs is None else pubs
        st = self.st if st is None else st
        tabs = [p3.Table.from_canonical(a, r, pv) for a, r, pv in zip(X.airs(st), rows, pubs)]
        q = o.oracle_p3_prove(tabs, st.init)
        a, b = o.oracle_p3_verify(tabs, q, st.init), p3.verify(tabs, q, st.init, params=self.blob)
        assert a == b
        return a


@pytest.fixture(scope="module")
def forge():
    f = Forge()
    yield f
    o.oracle_set_params()


@pytest.fixture(autouse=True)
def _forge_params(request):
    if "forge" in request.fixturenames:
        case, queries, init, more = FORGE
        preset, over, _, _ = P3_CASES[case]
        o.oracle_set_params(preset, **dict(over, queries=queries, **more))
    yield
    o.oracle_set_params()


def test_tables_of_another_init_are_refused(forge):
    """The shard proof B of the same tables under another init: its six open-statement tables verify -- no table of that
    statement mentions init.  The eight tables with init A claimed in the transcript's public values are refused, with B's
    chain rows (the first row absorbs B's init, not the public one: a constraint) and with A's honest chain (every
    constraint holds, but A's indices are not those of B's fold rows: the cumulative sums)."""
    f = forge
    case, queries, init, more = FORGE
    init_b = init[:-1] + [init[-1] + 1]
    blob, tables, iw_b, pf_b = setup(o.oracle_set_params, case, queries, init_b, more)
    assert not np.array_equal(pf_b, f.pf)
    st_b = X.statement(tables, pf_b, iw_b, blob)
    assert st_b.shape == f.st.shape and X.heights(st_b) == X.heights(f.st) and st_b.ops == f.st.ops
    open_b = H.host_tables(st_b.opn)
    fp = o.oracle_p3_prove(open_b, st_b.opn.init)
    assert p3.verify(open_b, fp, st_b.opn.init, params=blob) == 0
    pubs_b = [FR.from_mont(v.astype(np.uint64)) for v in X.public_values(st_b)]
    rows_b = X.witness(st_b)
    assert f.verdict(rows_b, pubs_b, st_b) == 0
    # B's rows, A's init in the public values
    claimed = [p.copy() for p in pubs_b]
    claimed[4][: len(init)] = init
    assert f.bad_rows(rows_b, 4, claimed, st_b) == [0] and f.verdict(rows_b, claimed, st_b) == 3
    # A's honest chain beside B's query rows: every table satisfies its constraints
    mixed = X.witness(st_b, chain=f.st)
    pubs_m = pubs_b[:4] + [f.pubs[4]] + pubs_b[5:]
    assert [f.bad_rows(mixed, t, pubs_m, st_b) for t in range(8)] == [[]] * 8
    idx_a, idx_b = f.rows[5][1: queries + 1, f.bc.IDX], rows_b[5][1: queries + 1, f.bc.IDX]
    assert not np.array_equal(idx_a, idx_b)
    assert f.verdict(mixed, pubs_m, st_b) == 8


def test_forged_indices(forge):
    f, bc = forge, forge.bc
    assert f.verdict(f.rows) == 0
    L, Q = f.st.shape.log_max, f.st.shape.queries
    r = 3                                                        # query 2
    # an index bit flipped in the bits table, nothing else: VALUE is no longer the sum of its bits, IDX not their low part
    rows = f.copy()
    rows[5][r][bc.B + 1] ^= 1
    assert f.bad_rows(rows, 5) == [r] and f.verdict(rows) == 3
    # ... with IDX and VALUE redone from the bits: the row is fine in itself, but it receives a sample nobody sent and sends
    # an index the fold table does not take
    rows = f.copy()
    v = int(rows[5][r][bc.VALUE]) ^ 2
    assert v < P
    rows[5][r] = X.bits_row(r, v, L, f.st.plan.pow_bits)
    assert f.bad_rows(rows, 5) == [] and f.verdict(rows) == 8
    # an index changed in fold'' only, the fold rows of that query redone from it
    rec = f.st.fold.records.reshape(Q, -1).copy()
    rec[r - 1, 0] = p3.to_mont([int(p3.from_mont(rec[r - 1, :1])[0]) ^ 2])[0]
    forged = F.Statement(f.st.shape, f.st.fold.publics, rec, f.blob)
    fold = G.fold_rows(f.st.red, F.witness(forged)[0])
    fc = F.FoldCols(f.st.shape)
    rows = f.copy()
    rows[0] = np.concatenate([fold, fold[:, fc.SEL: fc.SEL + 1]], axis=1)
    R_ = f.st.shape.n_rounds
    assert int(rows[0][(r - 1) * R_][fc.IDX]) == int(f.rows[0][(r - 1) * R_][fc.IDX]) ^ 2
    assert f.verdict(rows) == 8


def test_forged_index_bit_under_the_other_matrix(params):
    """the first two forgeries of test_forged_indices once more under m4_0: still refused, for the same reasons"""
    f = Forge("m4_0")
    bc = f.bc
    assert int(f.blob.p2_m4) == 0 and f.verdict(f.rows) == 0
    r = 3
    rows = f.copy()
    rows[5][r][bc.B + 1] ^= 1
    assert f.bad_rows(rows, 5) == [r] and f.verdict(rows) == 3
    rows = f.copy()
    v = int(rows[5][r][bc.VALUE]) ^ 2
    assert v < P
    rows[5][r] = X.bits_row(r, v, f.st.shape.log_max, f.st.plan.pow_bits)
    assert f.bad_rows(rows, 5) == [] and f.verdict(rows) == 8


def test_forged_public_values(forge):
    """one word of a beta, of a commit-phase root, of the final polynomial and of the proof-of-work witness changed in the
    transcript's public values only: the row that absorbs or gives it no longer holds it"""
    f = forge
    st = f.st
    n_perm = sum(m.batch == 1 for m in st.opn.layout)
    seg = X.observed_segments(st, f.iw.size, [int(t.public_values.size) for t in f.tables])
    assert seg is not None and n_perm
    beta1 = st.plan.n_obs + 8 + 12 + 4 + 2                       # behind pa, pb, alpha, zeta, alpha2 and beta of round 0
    for at in (beta1, seg["commit_roots"][0] + 8 + 3, seg["final_poly"][0] + 1, seg["witness"][0]):
        pubs = [p.copy() for p in f.pubs]
        pubs[4][at] = (int(pubs[4][at]) + 1) % P
        assert len(f.bad_rows(f.rows, 4, pubs)) == 1 and f.verdict(f.rows, pubs) == 3
    # the same words are the fold table's: verify_transcript_statement compares them
    assert np.array_equal(st.transcript_publics[beta1 - 2: beta1 + 2], st.fold.publics[4:8])


def test_forged_bits_rows(forge):
    f, bc = forge, forge.bc
    L, pw = f.st.shape.log_max, f.st.plan.pow_bits
    assert pw > 0
    # a proof-of-work row whose sample has a non-zero low bit
    rows = f.copy()
    v = int(rows[5][0][bc.VALUE]) | 1
    rows[5][0] = X.bits_row(0, v, L, pw)
    assert rows[5][0][bc.IDX] == 1 and f.bad_rows(rows, 5) == [0] and f.verdict(rows) != 0
    rows[5][0][bc.IDX] = 0                                       # ... and with IDX = 0 claimed: it is not the low bits
    assert f.bad_rows(rows, 5) == [0] and f.verdict(rows) != 0
    # VALUE + p in the bits, where that is below 2^31: the same field element, another index.  Against the AIR directly:
    # a trace of an honest proof-of-work row and one query row
    air = X.bits_air(L, pw)
    value = (1 << 26) + 12345
    assert value + P < 1 << 31
    trace = np.zeros((2, bc.width), dtype=np.uint64)
    trace[0], trace[1] = X.bits_row(0, 5 << pw, L, pw), X.bits_row(1, value, L, pw)
    assert air.check_trace(trace) == []
    big = value + P
    for i in range(31):
        trace[1][bc.B + i] = (big >> i) & 1
    trace[1][bc.H] = 1
    trace[1][bc.IDX] = big & ((1 << L) - 1)
    assert trace[1][bc.IDX] == (value + 1) & ((1 << L) - 1) and sum(int(trace[1][bc.B + i]) << i for i in range(31)) % P == value
    bad = air.check_trace(trace)
    assert [r for r, _ in bad] == [1] and len(bad) == 1          # the canonical form alone
    # ... and in a whole statement, where a sample is small enough
    small = [s for s in range(1, f.st.shape.queries + 1) if int(f.rows[5][s][bc.VALUE]) + P < 1 << 31]
    if small:
        s = small[0]
        rows = f.copy()
        big = int(rows[5][s][bc.VALUE]) + P
        for i in range(31):
            rows[5][s][bc.B + i] = (big >> i) & 1
        rows[5][s][bc.H], rows[5][s][bc.IDX] = 1, big & ((1 << L) - 1)
        assert f.bad_rows(rows, 5) == [s] and f.verdict(rows) != 0


# ---------------------------------------------------------------------------------------------- the lane bodies on the CPU
def step_words(plan):
    """the plan as rk_fri_transcript_rows_device uploads it (p3_kernels.hpp)"""
    out = []
    for s in plan.steps:
        out += [s.n_in, s.obs_off] + [s.bits[j] + 1 if j in s.bits else 0 for j in range(8)]
    return np.array(out, dtype=np.uint32)


@pytest.mark.parametrize("case", ["sp1_mixed_fib8_cubic4", "sp1_lookup_beside_plain", "sp1_same_height"] + PS.ROW_IDS,
                         ids=lambda c: c if isinstance(c, str) else PS.row_id(*c))
def test_kernel_lanes_on_the_cpu(params, tmp_path, case):
    so = str(tmp_path / "libemul_fri_transcript.so")
    src = os.path.join(o.EMUL_DIR, "emul_fri_transcript.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(o.ROOT, "raiko_amd", "csrc"), "-o", so, src],
                   check=True, capture_output=True)
    lib = C.CDLL(so)
    if isinstance(case, tuple):            # a set of tests/fri_param_sets.py: fri_transcript_chain_lane<0>, other tables, another field
        blob, tables, iw, pf = PS.cpu_shard(*case, transcript=True)
    else:
        queries, init, more = FULL[case]
        blob, tables, iw, pf = setup(params, case, queries, init, more)
    st = X.statement(tables, pf, iw, blob)
    want = [p3.to_mont(r) for r in X.witness(st)]
    rc_ext, rc_int, diag, m4 = R.tables_of()
    assert m4 == int(blob.p2_m4)
    tab = p3.to_mont(np.concatenate([rc_ext.reshape(-1), rc_int, diag]))
    sh = st.shape
    fold, trn, bits, state = (np.zeros_like(want[k]) for k in (0, 4, 5, 7))
    n_sponge = sh.queries * st.opn.perms_per_query
    state_in = np.zeros((state.shape[0], 16), dtype=np.uint32)
    state_mult = np.zeros(state.shape[0], dtype=np.uint32)
    state_in[:n_sponge], state_mult[:n_sponge] = want[7][:n_sponge, :16], want[7][:n_sponge, -1]
    mont = lambda v: int(p3.to_mont([v])[0])
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    steps = step_words(st.plan)
    lib.emul_fri_transcript_rows(sh.log_max, sh.blowup_log2, sh.queries, mont(pow(sh.root_2_27, 1 << (27 - sh.log_max), P)), mont(st.ext_w),
                                 mont(st.opn.coset_shift), vp(st.fold.publics), vp(st.fold.records), len(st.plan.steps), st.plan.pow_bits,
                                 C.c_size_t(n_sponge), vp(steps), vp(st.observed), vp(tab), m4, vp(fold), vp(trn), vp(bits), vp(state_in),
                                 vp(state_mult), vp(state), C.c_size_t(state.shape[0]))
    fc = F.FoldCols(sh)
    fold[:, fc.DIG: fc.DIG + 8] = want[0][:, fc.DIG: fc.DIG + 8]            # the leaf digests are the path lanes'
    for g_, w in zip((fold, trn, bits, state), (want[0], want[4], want[5], want[7])):
        assert np.array_equal(g_, w), np.argwhere(g_ != w)[:8]
