"""The commit form of the rv32im-mem chip set on the CPU (raiko_amd/rv32commit.py, rk_exec_commit_reads): every AIR
satisfied and every bus balanced on honest shards with the verifier's claims added, the lane bodies of rv32_rows.hpp
against numpy word for word, the journal cut from the logs the executor's byte for byte, commit=False unchanged, the
keyword refused where it does not belong, the chain check, and forged witnesses refused -- each by a named constraint, a
bus or the verifier's own checks -- with the honest twin accepted by the same code (`_accepts`).  The hole, shown once: a
journal that differs in one byte is nobody's business under io=True and is refused under commit=True."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rv32_commit_programs as CP
import test_rv32_io as TI
import test_rv32_mem_chips as T
from raiko_amd import _lib, p3, rv32, rv32_sets, rv32commit as RC, rv32elf, rv32im, rv32io, rv32link, rv32mem
from raiko_amd import executor as X
from raiko_amd.rv32commit import (Q_AD_LO, Q_AQ, Q_C0, Q_C1, Q_CNT, Q_CW, Q_HEAD, Q_JL, Q_JL4, Q_JPOS, Q_REM, Q_RINV, Q_RMH, Q_RMH7, Q_RML,
                                  Q_S, Q_S0, Q_T0B, Q_T1B, Q_V_LO, Q_Z)
from raiko_amd.segment import P

ROOT = T.ROOT
_runs = {}


def _run(name):
    if name not in _runs:
        fn, words = CP.RUNS[name]
        elf = fn()
        ex = X.execute(elf, list(words), segment_limit_po2=13, record_trace=True)
        image = rv32elf.program_image(elf)
        _runs[name] = (elf, ex, image, rv32io.preps_of(image), list(words))
    return _runs[name]


def _shards(ex):
    return zip(ex.segments, ex.witness, ex.rv32, ex.mem, ex.ecall_args, ex.commit_reads)


def _tables(name, k=0, link=False):
    """shard k of a run -> (canonical tables, public values per table, cycles, preps, the run's input)"""
    _elf, ex, image, preps, words = _run(name)
    s, (_c, data), (start, end, ecalls), mem, (args, pos), (reads, jpos) = list(_shards(ex))[k]
    canon, pc, pr, digest, iop = RC.shard_tables(s, data, start, end, ecalls, image, mem, args, reads, len(words), pos, jpos, link=link)
    return canon, [pc, (), pr] + [()] * 5 + [p3.from_mont(digest) if link else (), iop], s.cycles, preps, words


@pytest.fixture(scope="module")
def airs():
    return RC.airs()


@pytest.fixture(scope="module")
def linked_airs():
    return RC.airs(link=True)


def _accepts(airs, canon, preps, pubs, cycles, input_words, why=None, log=None, expected_journal=None):
    """what a proof of these tables would have to pass: every AIR, every bus balanced once the verifier's claims stand
    against BUS_INPUT and BUS_COMMIT, and the verifier's checks of the io public values and of the log it is handed.  log
    None: the prover hands over the log of ITS table with the digest to match (the forger's best case); else the digest in
    the public values must be the log's"""
    why = {} if why is None else why
    canon_pubs = list(pubs[:9]) + [p3.from_mont(pubs[9])]
    why["air"] = T._check(airs, canon, preps, canon_pubs, cpu_rows=cycles)
    bad = airs[9].check_trace(canon[9], canon_pubs[9])
    if bad:
        why["air"][9] = T._named(airs[9], bad)
    bal = RC.bus_balance(T._joined(canon, preps), airs)
    bal.pop(rv32link.BUS_LINK, None)
    sent_in, sent = bal.pop(rv32io.BUS_INPUT, {}), bal.pop(RC.BUS_COMMIT, {})
    why["bus"] = {b: v for b, v in bal.items() if v}
    pub = RC.publics_of(pubs[9])
    words = rv32io.slice_of(pub, input_words)
    why["publics"] = words is None
    if words is not None:
        why["claims in"] = sent_in != TI._stripped(rv32link.journal_tuples(rv32io.stream_journal(pub["pos_start"], words)))
    lg = canon[9].shape[0].bit_length() - 1
    handed = log is not None
    if not handed:
        log = RC.log_of_table(canon[9])
    got = RC.log_bytes(pub, log)
    why["log"] = got is None
    if handed and got is not None:                             # the verifier's order: the log's shape, then its digest
        why["digest"] = not np.array_equal(RC.log_root(log, lg), pub["commit_digest"])
    why["claims"] = sent != TI._stripped(rv32link.journal_tuples(log))
    if expected_journal is not None:
        why["journal"] = got != expected_journal
    return not any(why.values())


# ------------------------------------------------------------------------------------------------ registration
def test_commit_is_a_keyword_of_the_io_form_only(airs):
    from raiko_amd import p3_exec
    for kw in (dict(chips="rv32im-mem"), dict(chips="rv32im-mem", link=True), dict(chips="rv32im-elf", io=False), dict(chips="rv32i"),
               dict(chips="trace")):
        with pytest.raises(ValueError):
            p3_exec.execute_and_prove_p3(b"", commit=True, **kw)
        with pytest.raises(ValueError):
            p3_exec.P3Pipeline(commit=True, **kw)
    with pytest.raises(ValueError):
        rv32_sets._rv32_airs_of("rv32im-mem", commit=True)
    with pytest.raises(ValueError):
        rv32_sets.setup_rv32_elf(None, b"", chips="rv32im-mem", commit=True)
    with pytest.raises(ValueError):
        rv32_sets.rv32_shard_device(None, None, 0, None, (), chips="rv32im-mem", commit=True)
    with pytest.raises(ValueError):
        rv32_sets.execute_rv32_device(None, b"", chips="rv32im-mem", link=True, commit=True)
    with pytest.raises(ValueError):
        rv32mem.memop_air(commit=True)
    _elf, ex, image, _p, words = _run("small")
    with pytest.raises(ValueError):
        rv32_sets.shards("rv32im-mem", ex, image, commit=True)
    got = rv32_sets._rv32_airs_of("rv32im-mem", io=True, commit=True)
    assert [a.width for a in got] == [148, 1, rv32.REG_COLS, 1, 1, 1, 78, 65, 13, 64] == [a.width for a in airs]
    assert [a.prep_width for a in got] == [0, 48, 0, 4, 1, 4, 0, 0, 0, 0]                  # the io form's key: the decode is the same
    assert [a.n_public for a in got] == [4, 0, 128, 0, 0, 0, 0, 0, 0, 24]
    both = rv32_sets._rv32_airs_of("rv32im-mem", link=True, io=True, commit=True)
    assert both[8].n_public == 8 and len(both) == 10
    for a in got:
        assert a.log_quotient_degree() <= 1                 # every constraint has degree <= 3
        a.handle()
    # commit=False: the io form's AIRs, step for step
    plain, io = rv32_sets._rv32_airs_of("rv32im-mem", io=True), rv32io.airs()
    assert all(np.array_equal(a.steps, b.steps) and a.width == b.width and a.n_public == b.n_public for a, b in zip(plain, io))
    assert np.array_equal(plain[7].steps, rv32mem.memop_air(io=True, commit=False).steps) and plain[7].width == 64
    assert "bool ecr" in got[7].constraint_names and "bool ecr" not in plain[7].constraint_names
    assert rv32_sets._BY_COUNT[True, 10] is rv32_sets._IO   # a verifier tells the form by the public-value count
    assert RC.BUS_COMMIT == 14 and RC.ECR_CODE == 17 and RC.IO_TABLE == 9


# ------------------------------------------------------------------------------------------------ honest shards
@pytest.fixture(scope="module")
def commit_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_rv32_commit") / "libemul_rv32_commit.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", "emul_rv32_commit.cpp")], check=True, capture_output=True)
    return C.CDLL(so)


@pytest.mark.parametrize("name", sorted(CP.RUNS))
def test_honest_shards_satisfy_every_air_and_bus_and_the_lane_bodies_write_them(name, linked_airs, commit_lib):
    _elf, ex, _image, preps, words = _run(name)
    ptr = lambda a: a.ctypes.data_as(_lib.u32p)
    want = CP.expected_journal(name)
    assert ex.journal == want and len(ex.segments) == (3 if name == "three" else 1)
    proven, pubs_all = b"", []
    for k, (s, (_c, data), (_start, _end, ecalls), mem, (args, pos), (reads, jpos)) in enumerate(_shards(ex)):
        canon, pubs, cycles, _p, _w = _tables(name, k, link=True)
        why = {}
        assert _accepts(linked_airs, canon, preps, pubs, cycles, words, why), (name, k, why)
        pub = RC.publics_of(pubs[9])
        log = RC.log_of_table(canon[9])
        assert _accepts(linked_airs, canon, preps, pubs, cycles, words, log=log)           # ... and with the log handed over: its digest
        assert pub["jpos_start"] == jpos == len(proven) and log.shape[0] == reads.shape[0] == canon[9][:, Q_CW].sum()
        proven += RC.log_bytes(pub, log)
        assert pub["jpos_end"] == len(proven)
        pubs_all.append(pub)
        n_act = int(canon[9][:, rv32io.Q_ACT].sum())
        assert canon[9].shape[0] == max(2, 1 << int(n_act - 1).bit_length()) and n_act == len(args) + len(reads) + canon[9][:, rv32io.Q_WORD].sum()
        # rk_exec_mem_accesses holds none of the commit reads, the merged list all of them as ECR rows
        is_commit = np.isin(mem[:, 0], args[args[:, 1] == 2, 0]) if len(mem) else np.zeros(0, dtype=bool)
        assert not is_commit.any() and canon[7][:, rv32mem.G_ECR].sum() == len(reads) and canon[7][:, rv32mem.G_MULT].sum() == len(mem) + len(reads)
        # the lane bodies
        tr = rv32.trace_of(s, data)[0]
        rows = np.ascontiguousarray(np.stack([tr[c] for c in ("pc", "ins", "a", "b", "res", "next", "wr")], axis=1), dtype=np.uint32)
        out = [np.full(canon[i].shape, 0xDEADBEEF, dtype=np.uint32) for i in (7, 9)]
        got_log, n_log = np.full((canon[9].shape[0], 3), 0xDEADBEEF, dtype=np.uint32), C.c_size_t(0)
        ec, ea, acc, rd = (np.ascontiguousarray(a, dtype=np.uint32) for a in (ecalls, args, mem, reads))
        rc = commit_lib.emul_rv32commit_shard(ptr(rows), C.c_size_t(rows.shape[0]), ptr(ec), ptr(ea), C.c_size_t(ec.shape[0]), ptr(acc),
                                              C.c_size_t(acc.shape[0]), ptr(rd), C.c_size_t(rd.shape[0]), C.c_uint32(len(words)), C.c_uint32(pos),
                                              C.c_uint32(jpos), ptr(out[0]), C.c_size_t(out[0].shape[0]), ptr(out[1]),
                                              C.c_size_t(out[1].shape[0]), ptr(got_log), C.byref(n_log))
        assert rc == 0
        for g, i in zip(out, (7, 9)):
            assert np.array_equal(g, p3.to_mont(canon[i])), (name, k, i)
        assert n_log.value == log.shape[0] and np.array_equal(got_log[: n_log.value], log) and not got_log[n_log.value:].any()
        ok = lambda a, r, m: commit_lib.emul_rv32commit_list_ok(ptr(a), C.c_size_t(a.shape[0]), ptr(r), C.c_size_t(r.shape[0]), ptr(m),
                                                                C.c_size_t(m.shape[0]))
        assert ok(ea, rd, acc) == 1
        if len(rd) > 1:
            assert ok(ea, np.ascontiguousarray(rd[::-1]), acc) == 0 and ok(ea, rd[:-1], acc) == 0
            other = rd.copy()
            other[0, 1] += 1
            assert ok(ea, other, acc) == 0
            stray = np.array([[rd[0, 0], rd[0, 1], 0, 0]], dtype=np.uint32)               # an access at a COMMIT's cycle
            assert ok(ea, rd, stray) == 0
    assert proven == want == ex.journal
    assert RC.check_commit_chain(pubs_all) == len(want)
    assert rv32io.check_io_chain(pubs_all, words) == (ex.exit_code, ex.input_words_read)
    heights = {"small": 32, "big": 256, "many": 512, "edge": 8}
    if name in heights:
        assert canon[9].shape[0] == heights[name]
    if name == "three":                                      # shard 1 has no ecall: padding only, JPOS carried through
        canon1, pubs1 = _tables(name, 1)[:2]
        assert not canon1[9][:, rv32io.Q_ACT].any() and (canon1[9][:, Q_JPOS] == 6).all() and canon1[9].shape[0] == 2
        assert [(p["jpos_start"], p["jpos_end"]) for p in pubs_all] == [(0, 6), (6, 6), (6, 11)]


def test_guests_cover_every_case():
    io = _tables("small")[0][9]
    cw = io[io[:, Q_CW] == 1]
    sc = list(zip(cw[:, Q_S].tolist(), cw[:, Q_CNT].tolist()))
    assert sc == [(0, 1), (1, 1), (2, 1), (3, 1), (3, 1), (0, 1), (0, 4), (1, 3), (0, 4), (0, 4), (0, 4), (0, 1)]
    heads = io[io[:, Q_HEAD] == 1]
    assert heads[0, rv32io.Q_COMMIT] == 1 and heads[0, Q_REM] == 0 and io[1, Q_HEAD] == 1      # the 0-byte COMMIT: no row follows
    edge = _tables("edge")[0][9]
    e = edge[edge[:, Q_CW] == 1]
    assert e[:, rv32io.Q_K].tolist() == [0, 0, 1, 0] and e[:, rv32io.Q_AD_HI].tolist() == [0x30, 0x30, 0x31, 0x31]
    rd = _tables("read")[0]
    assert rd[9][:, rv32io.Q_WORD].sum() == 4 and rd[9][:, Q_CW].sum() == 4 and rd[7][:, rv32mem.G_SEL + 8].sum() == 4
    sb = _tables("sb")[0]
    w = sb[9][sb[9][:, Q_CW] == 1]
    assert w[0, rv32io.Q_AD_LO] == w[1, rv32io.Q_AD_LO] == w[2, rv32io.Q_AD_LO] and w[0, rv32io.Q_V_HI] != w[1, rv32io.Q_V_HI]
    assert sb[8][:, rv32mem.B_REAL].sum() == 1                # one word, four accesses
    big = _tables("big")[0][9]
    first = int(np.nonzero(big[:, Q_CW] == 1)[0][0])
    assert big[first - 1, Q_REM] == 513 and big[first:first + 129, Q_CW].all() and first + 129 > 128 and big[first, Q_S] == 3
    many = _tables("many")[0][9]
    assert many[:, Q_HEAD].sum() == 131 and many[:, Q_CW].sum() == 130


def test_commit_false_tables_are_rv32ios():
    _elf, ex, image, _preps, words = _run("read")
    plain = rv32_sets.shards("rv32im-mem", ex, image, io=True, input_words=words)
    for (tables, _init), (s, (_c, data), (start, end, ecalls), mem, (args, pos), _r) in zip(plain, _shards(ex)):
        want, _pc, _pr, _d, iop = rv32io.shard_tables(s, data, start, end, ecalls, image, mem, args, len(words), pos)
        assert len(tables) == 10 and all(np.array_equal(t.trace, p3.to_mont(w)) for t, w in zip(tables, want))
        assert np.array_equal(tables[9].public_values, iop) and iop.size == 14 and tables[7].trace.shape[1] == 64
    both = rv32_sets.shards("rv32im-mem", ex, image, io=True, input_words=words, commit=True)
    assert both[0][0][9].public_values.size == 24 and both[0][0][7].trace.shape[1] == 65 and len(both[0]) == 3


def test_chain_check():
    pubs = [RC.publics_of(_tables("three", k)[1][9]) for k in range(3)]
    assert RC.check_commit_chain(pubs) == 11 and RC.check_commit_chain(pubs[:2]) == 6 and RC.check_commit_chain([]) == 0
    gap, overlap = [dict(p) for p in pubs], [dict(p) for p in pubs]
    gap[2]["jpos_start"] = 7
    overlap[1]["jpos_start"] = overlap[1]["jpos_end"] = 5
    for bad, shard in ((gap, "shard 2"), (overlap, "shard 1"), (pubs[1:], "shard 0")):
        with pytest.raises(ValueError, match=shard):
            RC.check_commit_chain(bad)
    with pytest.raises(ValueError, match="shard 0"):
        RC.check_commit_chain([dict(pubs[0], jpos_end=1 << 30)])


# ------------------------------------------------------------------------------------------------ forgeries
def _set_cnt(t, r, cnt, slack):
    t[r, Q_CNT], t[r, Q_C0], t[r, Q_C1], t[r, Q_T0B], t[r, Q_T1B] = cnt, (cnt - 1) & 1, (cnt - 1) >> 1, slack & 1, slack >> 1


def _set_rem(t, r, rem):
    t[r, Q_REM], t[r, Q_RML], t[r, Q_RMH] = rem, rem & 0xFFFF, rem >> 16
    t[r, Q_RMH7], t[r, Q_Z], t[r, Q_RINV] = 128 * t[r, Q_RMH], int(rem == 0), rv32im._inv(np.array([rem]))[0]


def test_forged_commits_are_refused(airs):
    canon, pubs, cycles, preps, words = _tables("small")
    ok = lambda c, pv=pubs, why=None, **kw: _accepts(airs, c, preps, pv, cycles, words, why, **kw)
    assert ok(canon)
    io = canon[9]
    cws = np.nonzero(io[:, Q_CW] == 1)[0]
    r7, r9 = int(cws[7]), int(cws[9])                          # row 0 of the 7 bytes from offset 1; row 0 of the 9 bytes from offset 0
    last9 = r9 + 2

    def refused(fn, table=None, name=None, bus=None, pv=None):
        c = [t.copy() for t in canon]
        fn(c)
        why = {}
        assert not ok(c, pv if pv is not None else pubs, why=why)
        if name is not None:
            assert any(n == name for _r, n in why["air"].get(table, ())), (name, why["air"])
        if bus is not None:
            assert why["bus"].get(bus), (bus, list(why["bus"]))
        return why

    # a log word that is not memory's: the io row says so, the memop row that answers it holds memory's word
    def word(c):
        c[9][r9, Q_V_LO] ^= 1
    why = refused(word, bus=rv32mem.BUS_MEMOP)
    assert 9 not in why["air"] and not why["claims"]          # the log follows the forged table: the memory argument refuses
    # S is not a0 & 3
    def start(c):
        c[9][r7, Q_S], c[9][r7, Q_S0] = 0, 0
        _set_cnt(c[9], r7, 3, 1)
    refused(start, 9, "first lo cw")
    def start_later(c):
        c[9][r7 + 1, Q_S], c[9][r7 + 1, Q_S0] = 1, 1
        _set_cnt(c[9], r7 + 1, 3, 0)
    refused(start_later, 9, "s later")
    # a middle row that stops short of its word's end
    def short(c):
        _set_cnt(c[9], r9, 3, 1)
        _set_rem(c[9], r9, 6)
    refused(short, 9, "full")
    # CNT = 0
    def none(c):
        c[9][r9, Q_CNT] = 0
    refused(none, 9, "cnt")
    def none_bits(c):                                          # ... with the slack following: the bits cannot say 0
        c[9][r9, Q_CNT], c[9][r9, Q_T0B], c[9][r9, Q_T1B] = 0, 0, 2
    assert {n for _r, n in refused(none_bits)["air"][9]} & {"cnt", "bool t1b"}
    # a CNT above what is left: REM = -1 satisfies the countdown in the field and has no limbs below 2^25
    def over(c):
        _set_cnt(c[9], last9, 2, 2)
        _set_rem(c[9], last9, P - 1)
    why = refused(over, bus=rv32.BUS_RANGE16)
    assert not {n for _r, n in why["air"][9]} & {"rem bytes", "rem limbs", "fit"}
    # one row too few, one too many
    def dropped(c):
        c[9][last9:-1] = c[9][last9 + 1:].copy()
    assert {n for _r, n in refused(dropped)["air"][9]} & {"word follows", "rem bytes"}
    def doubled(c):
        c[9][last9 + 1:] = c[9][last9:-1].copy()
    assert {n for _r, n in refused(doubled)["air"][9]} & {"word follows", "cw kind", "rem bytes"}
    # a commit-word row after the COMMIT of 0 bytes
    def after_none(c):
        c[9][2:] = c[9][1:-1].copy()
        c[9][1] = c[9][cws[0]]
        c[9][1, rv32io.Q_TS] = c[9][0, rv32io.Q_TS]
    refused(after_none, 9, "word follows")
    # JPOS skips, rewinds
    for d in (1, -1):
        def jpos(c, d=d):
            c[9][r9:, Q_JPOS] += d
            c[9][r9:, Q_JL] += d * c[9][r9:, Q_CW]
            c[9][r9:, Q_JL4] += 4 * d * c[9][r9:, Q_CW]
        refused(jpos, 9, "jpos")
    # a wrong address step
    def step(c):
        c[9][r9 + 1, Q_AD_LO] += 4
        c[9][r9 + 1, Q_AQ] += 1
    refused(step, 9, "next lo")
    # JPOS_START, JPOS_END forged
    for at, name in ((RC.PUB_JPOS_START, "jpos start"), (RC.PUB_JPOS_END, "jpos end")):
        pv = list(pubs)
        canon_pub = p3.from_mont(pubs[9][:RC.PUB_COMMIT_DIGEST]).astype(np.int64)
        canon_pub[at] += 1
        pv[9] = np.concatenate([p3.to_mont(canon_pub), pubs[9][RC.PUB_COMMIT_DIGEST:]])
        refused(lambda c: None, 9, name, pv=pv)
    # an ECR row that changes memory
    def writes(c):
        m = c[7]
        r = int(np.nonzero(m[:, rv32mem.G_ECR] == 1)[0][0])
        m[r, rv32mem.G_N] ^= 1
        m[r, rv32mem.G_N_LO] ^= 1
        m[r, rv32mem.G_AND + 2] = m[r, rv32mem.G_N] & m[r, rv32mem.G_N + 1]
    refused(writes, 7, "load keeps 0")
    # an ECR row that reports another word than memory holds
    def lies(c):
        m = c[7]
        r = int(np.nonzero(m[:, rv32mem.G_ECR] == 1)[0][0])
        m[r, rv32mem.G_R_LO] ^= 1
    refused(lies, 7, "lw lo")
    # a log handed to the verifier with one byte changed; a log of another shape
    log = RC.log_of_table(io)
    assert ok(canon, log=log, expected_journal=CP.expected_journal("small"))
    other = log.copy()
    other[3, 1] ^= 0x01000000
    why = {}
    assert not ok(canon, log=other, why=why) and why["digest"] and why["claims"] and not why["log"]
    for bad in (log[:-1], np.concatenate([log[:1], log])):
        why = {}
        assert not ok(canon, log=bad, why=why) and why["log"]
    wide = log.copy()
    wide[0, 2] = 3 | 2 << 16                                   # S + CNT = 5
    why = {}
    assert not ok(canon, log=wide, why=why) and why["log"]


def test_verifier_refuses_a_foreign_log_before_the_proof_is_read():
    """verify_rv32_shard with a proof of which only the header's heights are real: reason 2 for a log with one byte
    changed, a log of another shape, and public values that do not fit it"""
    _elf, ex, image, _preps, words = _run("small")
    tables, init, log = rv32_sets.shards("rv32im-mem", ex, image, io=True, input_words=words, commit=True)[0]
    proof = np.zeros(64, dtype=np.uint32)
    proof[1:11] = [t.log_height for t in tables]
    root, plh = np.zeros(8, dtype=np.uint32), tables[1].log_height
    other = log.copy()
    other[5, 1] ^= 1
    for bad in (other, log[:-1], log[1:]):
        assert rv32_sets.verify_rv32_shard(tables, proof, init, None, root, plh, input_words=words, commit_log=bad) == 2
    with pytest.raises(ValueError):
        rv32_sets.verify_rv32_shard(tables, proof, init, None, root, plh, input_words=words)          # 24 public values go with a log
    with pytest.raises(ValueError):
        rv32_sets.verify_rv32_shard(tables, proof, init, None, root, plh, commit_log=log)
    io_tables, io_init = rv32_sets.shards("rv32im-mem", ex, image, io=True, input_words=words)[0]
    with pytest.raises(ValueError):
        rv32_sets.verify_rv32_shard(io_tables, proof, io_init, None, root, plh, input_words=words, commit_log=log)   # 14: the io form
    with pytest.raises(ValueError):
        rv32_sets.verify_rv32_execution([(tables, init)], [proof], commit_logs=[log])                 # ... and input_words
    with pytest.raises(ValueError):
        rv32_sets.verify_rv32_execution([(tables, init)], [proof], input_words=words, expected_journal=b"")


def test_the_hole_a_journal_that_differs_in_one_byte(airs):
    """under io=True nothing a proof checks names the journal: the statement is accepted whatever journal comes with it.
    Under commit=True the verifier cuts the journal from the log the proof is bound to"""
    want = CP.expected_journal("read")
    forged = bytes([want[0] ^ 1]) + want[1:]
    elf, ex, image, preps, words = _run("read")
    assert ex.journal == want
    s, (_c, data), (start, end, ecalls), mem, (args, pos), _r = list(_shards(ex))[0]
    canon, pc, pr, _d, iop = rv32io.shard_tables(s, data, start, end, ecalls, image, mem, args, len(words), pos)
    io_pubs = [pc, (), pr] + [()] * 5 + [(), iop]
    assert TI._accepts(rv32io.airs(), canon, preps, io_pubs, s.cycles, words)      # with `want` or with `forged`: nothing looks
    assert set(rv32io.publics_of(iop)) == {"pos_start", "pos_end", "n_input", "halted", "exit", "limbs", "digest"}
    canon, pubs, cycles, preps, words = _tables("read")
    assert _accepts(airs, canon, preps, pubs, cycles, words, expected_journal=want)
    why = {}
    assert not _accepts(airs, canon, preps, pubs, cycles, words, why, expected_journal=forged) and why["journal"]
