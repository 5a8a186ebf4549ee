"""The io and commit forms of the rv32im-mem chip set on the CPU where the io table's limbs carry (raiko_amd/rv32io.py,
raiko_amd/rv32commit.py; the guests of tests/rv32_limb_programs.py): journal positions past 2^14, a COMMIT of more than 2^16
bytes, stream positions and an input past 2^14 with the three-way carry at 1 and 2, a READ capacity of 2^16 and more with
its borrow, two heads more than 2^14 timestamps apart.  Honest shards: the lane bodies of rv32_rows.hpp against numpy
word for word, the journal cut from the logs, the chain checks; every AIR and bus (`_accepts` of test_rv32_commit.py) on
the shards whose io table has at most 2^13 rows, the io AIR alone on the taller ones (their acceptance as a whole is the
GPU proof of tests/test_gpu_rv32_io_limbs.py).  Starts no guest reaches, injected into io_rows and the lane bodies; the
journal's end at 2^30; and limb forgeries, each refused by a named constraint, RANGE16 or the verifier's own checks with
its honest twin accepted by the same code."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rv32_commit_programs as CP
import rv32_io_programs as IP
import rv32_limb_programs as LP
import test_rv32_commit as TC
import test_rv32_io as TI
import test_rv32_mem_chips as T
from raiko_amd import _lib, p3, rv32, rv32commit as RC, rv32elf, rv32io, rv32mem
from raiko_amd import executor as X
from raiko_amd.rv32 import BUS_RANGE16
from raiko_amd.rv32commit import (Q_B_HI, Q_B_LO, Q_BH7, Q_C, Q_COMMIT, Q_CW, Q_EH, Q_FHI, Q_FLO, Q_GAP_H, Q_GH, Q_HEAD, Q_JH, Q_JL, Q_JL4,
                                  Q_JPOS, Q_K, Q_KF, Q_NH, Q_NL, Q_NL4, Q_PH, Q_PL, Q_PL4, Q_POS, Q_READ, Q_REM, Q_RMH, Q_RMH7, Q_WORD)
from raiko_amd.segment import P

ROOT = T.ROOT
FULL_ROWS = 1 << 13                                         # `_accepts` up to here; the io AIR alone above
_runs, _tabs = {}, {}
ptr = lambda a: a.ctypes.data_as(_lib.u32p)


def _run(name):
    if name not in _runs:
        fn, words = LP.RUNS[name]
        elf = fn()
        ex = X.execute(elf, list(words), segment_limit_po2=LP.PO2[name], record_trace=True)
        image = rv32elf.program_image(elf)
        _runs[name] = (elf, ex, image, rv32io.preps_of(image), list(words))
    return _runs[name]


def _tables(name, k=0):
    """shard k of a run, linked -> (canonical tables, public values per table, cycles, preps, the run's input)"""
    if (name, k) not in _tabs:
        _elf, ex, image, preps, words = _run(name)
        s, (_c, data), (start, end, ecalls), mem, (args, pos), (reads, jpos) = list(TC._shards(ex))[k]
        canon, pc, pr, digest, iop = RC.shard_tables(s, data, start, end, ecalls, image, mem, args, reads, len(words), pos, jpos, link=True)
        _tabs[name, k] = canon, [pc, (), pr] + [()] * 5 + [p3.from_mont(digest), iop], s.cycles, preps, words
    return _tabs[name, k]


def _io(name, k=0):
    return _tables(name, k)[0][9]


@pytest.fixture(scope="module")
def linked_airs():
    return RC.airs(link=True)


def _build(tmp_path_factory, name):
    so = str(tmp_path_factory.mktemp(name) / ("lib%s.so" % name))
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", name + ".cpp")], check=True, capture_output=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def commit_lib(tmp_path_factory):
    return _build(tmp_path_factory, "emul_rv32_commit")


@pytest.fixture(scope="module")
def io_lib(tmp_path_factory):
    return _build(tmp_path_factory, "emul_rv32_io")


def _trace_rows(s, data):
    tr = rv32.trace_of(s, data)[0]
    return np.ascontiguousarray(np.stack([tr[c] for c in ("pc", "ins", "a", "b", "res", "next", "wr")], axis=1), dtype=np.uint32)


def _emul_commit(lib, rows, ecalls, args, mem, reads, n_input, pos, jpos, memop_rows, io_rows):
    """emul_rv32commit_shard -> (its return code, memop, io: Montgomery, the log: canonical, cut to its length)"""
    memop = np.full((memop_rows, rv32mem.MEMOP_COLS_COMMIT), 0xDEADBEEF, dtype=np.uint32)
    io = np.full((io_rows, RC.IO_COLS), 0xDEADBEEF, dtype=np.uint32)
    log, n_log = np.full((io_rows, 3), 0xDEADBEEF, dtype=np.uint32), C.c_size_t(0)
    ec, ea, acc, rd = (np.ascontiguousarray(a, dtype=np.uint32) for a in (ecalls, args, mem, reads))
    rc = lib.emul_rv32commit_shard(ptr(rows), C.c_size_t(rows.shape[0]), ptr(ec), ptr(ea), C.c_size_t(ec.shape[0]), ptr(acc),
                                   C.c_size_t(acc.shape[0]), ptr(rd), C.c_size_t(rd.shape[0]), C.c_uint32(n_input), C.c_uint32(pos),
                                   C.c_uint32(jpos), ptr(memop), C.c_size_t(memop_rows), ptr(io), C.c_size_t(io_rows), ptr(log),
                                   C.byref(n_log))
    if rc == 0:
        assert not log[n_log.value:].any()
    return rc, memop, io, log[: n_log.value]


def _io_publics(pubs):
    """io_rows' eight leading public values -> the 24 canonical ones, the digests (which no constraint reads) zero"""
    pv = np.zeros(RC.N_PUBLIC_IO, dtype=np.int64)
    pv[:rv32io.PUB_DIGEST] = pubs[:rv32io.PUB_DIGEST]
    pv[RC.PUB_JPOS_START], pv[RC.PUB_JPOS_END] = pubs[rv32io.PUB_DIGEST:]
    return pv


def _range16_accepts(t, hist, io_range=RC.IO_RANGE):
    """every limb the table sends to RANGE16 is a 16-bit value and the counts io_rows adds hold each of them"""
    sent = np.concatenate([t[t[:, m] == 1, c] for c, m in io_range])
    return bool((sent >= 0).all() and (sent < 1 << 16).all()) and np.array_equal(hist, np.bincount(sent, minlength=1 << 16))


# ------------------------------------------------------------------------------------------------ the guests
def _block0(io, block=128):
    """(io rows, commit words, commit bytes) of the table's first `block` ecalls: the three totals of block 0 of the scan"""
    heads = np.nonzero(io[:, Q_HEAD] == 1)[0]
    end = int(heads[block])
    return end, int(io[:end, Q_CW].sum()), int(io[end, Q_JPOS] - io[0, Q_JPOS])


def test_guests_cover_every_case():
    j14 = _io("j14")
    cw = j14[j14[:, Q_CW] == 1]
    assert j14.shape[0] == 8192 and len(cw) == 4096 + 3 and len(_run("j14")[1].segments) == 1
    assert cw[-3:, Q_JPOS].tolist() == [16381, 16383, 16387] and cw[-3:, Q_JH].tolist() == [0, 0, 1]      # inside the second call
    assert cw[-2, Q_JL] == 16383 and cw[-1, Q_JL] == 3 and cw[:, Q_JL4].max() == 4 * 16383
    for name in LP.RUNS:
        assert len(_run(name)[1].segments) == LP.SHARDS[name], name
    x0, x1 = _io("j14x"), _io("j14x", 1)
    pub1 = RC.publics_of(_tables("j14x", 1)[1][9])
    assert x0.shape[0] == 8192 and x0[:, Q_JH].max() == 0 and x1.shape[0] == 4 and (pub1["jpos_start"], pub1["jpos_end"]) == (16383, 16388)
    assert x1[x1[:, Q_CW] == 1][:, [Q_JL, Q_JH]].tolist() == [[16383, 0], [1, 1]] and x1[0, Q_JPOS] == 16383
    rem, rem_mo = _io("rem16"), _tables("rem16")[0][7]
    head = rem[rem[:, Q_COMMIT] == 1][0]
    cw = rem[rem[:, Q_CW] == 1]
    assert rem.shape[0] == rem_mo.shape[0] == 1 << 15 and _tables("rem16")[0][0].shape[0] == 1 << 14 and len(cw) == 16387
    assert (head[Q_B_HI], head[Q_B_LO], head[Q_BH7], head[Q_REM]) == (1, 5, 128, 65541)
    assert cw[0, Q_RMH] == 1 and cw[0, Q_RMH7] == 128 and cw[:2, Q_REM].tolist() == [65538, 65534] and cw[:, Q_JH].max() == 4
    assert cw[:, Q_K].sum() == 1 and rem_mo[:, rv32mem.G_ECR].sum() == 16387                    # one 2^16 address boundary
    c0, c1 = _io("carry2"), _io("carry2", 1)
    h0, h1 = c0[c0[:, Q_READ] == 1][0], c1[c1[:, Q_READ] == 1][0]
    assert c0.shape[0] == c1.shape[0] == 1 << 14
    assert (h0[Q_NH], h0[Q_EH], h0[Q_C], h0[Q_POS]) == (2, 1, 1, 0) and (h1[Q_NH], h1[Q_EH], h1[Q_C], h1[Q_POS]) == (2, 0, 2, 12000)
    w1 = c1[c1[:, Q_WORD] == 1]
    assert w1[0, Q_PH] == 0 and w1[-1, Q_PH] == 1 and w1[-1, Q_POS] == 23999 and w1[:, Q_PH].sum() == 24000 - 16384
    k1 = _io("carry1")
    reads = k1[k1[:, Q_READ] == 1]
    assert k1.shape[0] == 16 and reads[:, Q_NH].tolist() == [1, 1] and reads[:, Q_C].tolist() == [1, 1] and reads[:, Q_NL].tolist() == [4, 4]
    g = _io("got14")
    gh = g[g[:, Q_READ] == 1][0]
    assert g.shape[0] == 1 << 15 and gh[Q_GH] == 1 and gh[Q_C] == 0 and g[:, Q_PH].max() == 1 and g[g[:, Q_WORD] == 1][:, Q_K].sum() == 1
    cap = _io("cap16")
    r = cap[cap[:, Q_READ] == 1]
    assert r[:, Q_FHI].tolist() == [0, 2] and r[:, Q_FLO].tolist() == [0xFFFD, 0] and r[:, Q_KF].tolist() == [1, 0] and r[:, Q_REM].tolist() == [5, 0]
    gap = _io("gap14")
    gheads = gap[gap[:, Q_HEAD] == 1]
    assert gheads[:, Q_GAP_H].tolist() == [0, 1, 0] and gap.shape[0] == 8
    mixed = _io("mixed")
    calls = [LP.mixed_call(c) for c in range(128)]
    want_words = sum(RC.n_commit_words(a0, a1) for t0, a0, a1 in calls if t0 == 2)
    want = (128 + min(LP.MIXED_INPUT, sum(t0 == 1 for t0, _a, _b in calls)) + want_words, want_words, sum(a1 for t0, _a, a1 in calls if t0 == 2))
    assert _block0(mixed) == want and len(set(want)) == 3 and mixed[:, Q_HEAD].sum() == LP.MIXED_CALLS + 1 > 128
    short = mixed[(mixed[:, Q_READ] == 1) & (mixed[:, Q_REM] == 0)]
    assert len(short) == 47 - LP.MIXED_INPUT and mixed.shape[0] == 512
    # every high limb and carry is non-zero somewhere, and the three-way carry takes its three values
    tables = [_io(name, k) for name in LP.RUNS for k in range(LP.SHARDS[name])]
    for col in (Q_JH, Q_RMH, Q_RMH7, Q_PH, Q_NH, Q_EH, Q_GH, Q_FHI, Q_KF, Q_GAP_H):
        assert any(t[:, col].any() for t in tables), col
    assert any(t[t[:, Q_COMMIT] == 1][:, [Q_BH7, Q_B_HI]].all(axis=1).any() for t in tables)       # on a COMMIT head
    assert {int(c) for t in tables for c in t[t[:, Q_READ] == 1][:, Q_C]} == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ honest shards
@pytest.mark.parametrize("name", sorted(LP.RUNS))
def test_honest_shards_lane_bodies_journal_and_chain(name, linked_airs, commit_lib):
    _elf, ex, _image, preps, words = _run(name)
    want = LP.expected_journal(name)
    assert ex.journal == want and (ex.exit_code, ex.input_words_read) == LP.EXPECT[name]
    proven, pubs_all = b"", []
    for k, (s, (_c, data), (_start, _end, ecalls), mem, (args, pos), (reads, jpos)) in enumerate(TC._shards(ex)):
        canon, pubs, cycles, _p, _w = _tables(name, k)
        log = RC.log_of_table(canon[9])
        rc, memop, io, got_log = _emul_commit(commit_lib, _trace_rows(s, data), ecalls, args, mem, reads, len(words), pos, jpos,
                                              canon[7].shape[0], canon[9].shape[0])
        assert rc == 0 and np.array_equal(memop, p3.to_mont(canon[7])) and np.array_equal(io, p3.to_mont(canon[9])), (name, k)
        assert np.array_equal(got_log, log) and len(log) == len(reads), (name, k)
        if canon[9].shape[0] <= FULL_ROWS:
            why = {}
            assert TC._accepts(linked_airs, canon, preps, pubs, cycles, words, why, log=log), (name, k, why)
        else:
            canon_pub = p3.from_mont(pubs[9])
            assert linked_airs[9].check_trace(canon[9], canon_pub) == [], (name, k)
        pub = RC.publics_of(pubs[9])
        assert pub["jpos_start"] == jpos == len(proven) and pub["pos_start"] == pos
        assert np.array_equal(pub["commit_digest"], RC.log_root(log, canon[9].shape[0].bit_length() - 1))
        proven += RC.log_bytes(pub, log)
        assert pub["jpos_end"] == len(proven)
        pubs_all.append(pub)
    assert proven == want
    assert RC.check_commit_chain(pubs_all) == len(want)
    assert rv32io.check_io_chain(pubs_all, words) == LP.EXPECT[name]


@pytest.mark.parametrize("name", LP.READ_ONLY)
def test_read_only_guests_under_plain_io(name, io_lib):
    """the io form's lane bodies (47 columns, no journal position) on the guests that make no COMMIT"""
    _elf, ex, image, preps, words = _run(name)
    airs = rv32io.airs(link=True)
    pubs_all = []
    for k, (s, (_c, data), (start, end, ecalls), mem, (args, pos)) in enumerate(TI._shards(ex)):
        canon, pc, pr, digest, iop = rv32io.shard_tables(s, data, start, end, ecalls, image, mem, args, len(words), pos, link=True)
        rows = _trace_rows(s, data)
        out = [np.full(canon[i].shape, 0xDEADBEEF, dtype=np.uint32) for i in (0, 7, 9)]
        ec, ea, acc = (np.ascontiguousarray(a, dtype=np.uint32) for a in (ecalls, args, mem))
        rc = io_lib.emul_rv32io_shard(ptr(rows), C.c_size_t(rows.shape[0]), C.c_size_t(canon[0].shape[0]), C.c_uint32(s.end_pc),
                                      ptr(np.ascontiguousarray(start, dtype=np.uint32)), ptr(ec), ptr(ea), C.c_size_t(ec.shape[0]), ptr(acc),
                                      C.c_size_t(acc.shape[0]), C.c_uint32(len(words)), C.c_uint32(pos), ptr(out[0]), ptr(out[1]),
                                      C.c_size_t(out[1].shape[0]), ptr(out[2]), C.c_size_t(out[2].shape[0]))
        assert rc == 0
        for g, i in zip(out, (0, 7, 9)):
            assert np.array_equal(g, p3.to_mont(canon[i])), (name, k, i)
        assert np.array_equal(canon[9], _io(name, k)[:, :rv32io.IO_COLS])          # the commit form's table, its first 47 columns
        pubs = [pc, (), pr] + [()] * 5 + [p3.from_mont(digest), iop]
        if canon[9].shape[0] <= FULL_ROWS:                 # a taller one: the columns above, judged once under the commit form's AIR
            why = {}
            assert TI._accepts(airs, canon, preps, pubs, s.cycles, words, why), (name, k, why)
        pubs_all.append(rv32io.publics_of(iop))
    assert rv32io.check_io_chain(pubs_all, words) == LP.EXPECT[name]


# ------------------------------------------------------------------------------------------------ injected starts
def _shard0(run):
    _elf, ex, _image, _preps, words = run
    s, (_c, data), (_start, _end, ecalls), mem, (args, pos), (reads, jpos) = list(TC._shards(ex))[0]
    return _trace_rows(s, data), ecalls, np.asarray(args, dtype=np.int64), mem, reads, len(words)


SMALL_LEN = len(CP.expected_journal("small"))
JPOS_STARTS = [(1 << 14) - 2, (1 << 28) + 16383, (1 << 30) - 64, (1 << 30) - 1 - SMALL_LEN]


@pytest.mark.parametrize("jpos_start", JPOS_STARTS)
def test_injected_journal_starts(jpos_start, linked_airs, commit_lib):
    """the `small` guest of the commit form's tests as a shard that starts at journal positions no guest reaches; the
    last start ends the journal at 2^30 - 1, the largest end there is"""
    rows, ecalls, args, mem, reads, n_input = _shard0(TC._run("small"))
    t, hist, pubs = RC.io_rows(args, ecalls, mem, reads, n_input, 0, jpos_start)
    mo_rows = TC._tables("small")[0][7].shape[0]
    rc, _memop, io, log = _emul_commit(commit_lib, rows, ecalls, args, mem, reads, n_input, 0, jpos_start, mo_rows, t.shape[0])
    assert rc == 0 and np.array_equal(io, p3.to_mont(t)) and np.array_equal(log, RC.log_of_table(t))
    assert linked_airs[9].check_trace(t, _io_publics(pubs)) == [] and _range16_accepts(t, hist)
    cw = t[t[:, Q_CW] == 1]
    assert np.array_equal(cw[:, Q_JL] + (cw[:, Q_JH] << 14), cw[:, Q_JPOS]) and cw[0, Q_JPOS] == jpos_start and cw[:, Q_JL].max() < 1 << 14
    assert cw[:, Q_JH].max() == (jpos_start + SMALL_LEN - 1) >> 14
    pub = dict(jpos_start=jpos_start, jpos_end=int(pubs[-1]))
    assert pub["jpos_end"] == jpos_start + SMALL_LEN and RC.log_bytes(pub, log) == CP.expected_journal("small")


def test_a_journal_that_ends_at_2_to_30_is_refused_by_all_three(commit_lib):
    """numpy, the lane body (io_commit_head) and the verifier's log_bytes draw one line: a journal ends below 2^30"""
    rows, ecalls, args, mem, reads, n_input = _shard0(TC._run("small"))
    mo_rows, io_rows = TC._tables("small")[0][7].shape[0], TC._tables("small")[0][9].shape[0]
    t, _h, pubs = RC.io_rows(args, ecalls, mem, reads, n_input, 0, JPOS_STARTS[-1])
    last = RC.log_of_table(t)
    for start in ((1 << 30) - SMALL_LEN, (1 << 30) - 8, 1 << 30):
        with pytest.raises(ValueError, match="2\\^30"):
            RC.io_rows(args, ecalls, mem, reads, n_input, 0, start)
        assert _emul_commit(commit_lib, rows, ecalls, args, mem, reads, n_input, 0, start, mo_rows, io_rows)[0] == 5
        moved = last.astype(np.int64)
        moved[:, 0] += start - JPOS_STARTS[-1]              # the log such a shard would hand over
        assert RC.log_bytes(dict(jpos_start=start, jpos_end=start + SMALL_LEN), moved.astype(np.uint32)) is None
        with pytest.raises(ValueError, match="shard 0"):
            RC.check_commit_chain([dict(jpos_start=0, jpos_end=start + SMALL_LEN)])


@pytest.mark.parametrize("pos_start,n_input", [(16383, 16384 + 6), (1 << 29, (1 << 29) + 6)])
def test_injected_stream_starts(pos_start, n_input, linked_airs, commit_lib, io_lib):
    """guests that READ six words, shifted to stream positions no guest reaches: the commit form (`read`: a READ of 4 and
    a COMMIT) with a journal start past 2^14 as well, and the io form (`reads`: capacity 0, below, at and above what is left)"""
    rows, ecalls, args, mem, reads, n6 = _shard0(TC._run("read"))
    assert n6 == 6
    args = args.copy()
    args[:, 4] += pos_start
    jpos_start = (1 << 14) - 5
    t, hist, pubs = RC.io_rows(args, ecalls, mem, reads, n_input, pos_start, jpos_start)
    mo_rows = TC._tables("read")[0][7].shape[0]
    rc, _memop, io, log = _emul_commit(commit_lib, rows, ecalls, args, mem, reads, n_input, pos_start, jpos_start, mo_rows, t.shape[0])
    assert rc == 0 and np.array_equal(io, p3.to_mont(t)) and np.array_equal(log, RC.log_of_table(t))
    assert linked_airs[9].check_trace(t, _io_publics(pubs)) == [] and _range16_accepts(t, hist)
    head = t[t[:, Q_READ] == 1][0]
    words = t[t[:, Q_WORD] == 1]
    assert (head[Q_PL], head[Q_PH], head[Q_NL], head[Q_NH]) == (pos_start & 0x3FFF, pos_start >> 14, n_input & 0x3FFF, n_input >> 14)
    left = n_input - pos_start - 4                              # E: what the READ of 4 leaves
    assert head[Q_C] == ((pos_start & 0x3FFF) + 4 + (left & 0x3FFF)) >> 14 and words[:, Q_POS].tolist() == [pos_start + k for k in range(4)]
    assert (head[rv32io.Q_EL], head[Q_EH], head[rv32io.Q_ZR]) == (left, 0, 0)
    assert np.array_equal(words[:, Q_PL] + (words[:, Q_PH] << 14), words[:, Q_POS]) and words[:, Q_PL].max() < 1 << 14
    assert pubs[:3].tolist() == [pos_start, pos_start + 4, n_input] and t[t[:, Q_CW] == 1][:, Q_JH].max() == 1
    # the io form: `reads` exhausts its six words, so it starts six before the input's end
    pos_start = n_input - 6
    _elf, ex, _image, _preps, words6 = TI._run("reads")
    s, (_c, data), (start, _end, ecalls), mem, (args, pos) = list(TI._shards(ex))[0]
    args = np.asarray(args, dtype=np.int64).copy()
    args[:, 4] += pos_start
    t, hist, pubs = rv32io.io_rows(args, ecalls, mem, n_input, pos_start)
    canon = TI._tables("reads")[0]
    rows = _trace_rows(s, data)
    out = [np.full((canon[i].shape[0], w), 0xDEADBEEF, dtype=np.uint32) for i, w in ((0, canon[0].shape[1]), (7, canon[7].shape[1]), (9, rv32io.IO_COLS))]
    ec, ea, acc = (np.ascontiguousarray(a, dtype=np.uint32) for a in (ecalls, args, mem))
    rc = io_lib.emul_rv32io_shard(ptr(rows), C.c_size_t(rows.shape[0]), C.c_size_t(canon[0].shape[0]), C.c_uint32(s.end_pc),
                                  ptr(np.ascontiguousarray(start, dtype=np.uint32)), ptr(ec), ptr(ea), C.c_size_t(ec.shape[0]), ptr(acc),
                                  C.c_size_t(acc.shape[0]), C.c_uint32(n_input), C.c_uint32(pos_start), ptr(out[0]), ptr(out[1]),
                                  C.c_size_t(out[1].shape[0]), ptr(out[2]), C.c_size_t(out[2].shape[0]))
    assert rc == 0 and np.array_equal(out[2], p3.to_mont(t)) and t.shape[0] == canon[9].shape[0]
    pv = np.zeros(rv32io.N_PUBLIC_IO, dtype=np.int64)
    pv[:rv32io.PUB_DIGEST] = pubs
    assert rv32io.io_air().check_trace(t, pv) == [] and _range16_accepts(t, hist, rv32io.IO_RANGE)
    heads = t[t[:, Q_READ] == 1]
    assert heads[:, Q_REM].tolist() == [0, 2, 4, 0] and heads[:, Q_POS].tolist() == [pos_start + d for d in (0, 0, 2, 6)]
    assert heads[:, Q_C].tolist() == [((pos_start + d & 0x3FFF) + g + (6 - d - g & 0x3FFF)) >> 14 for d, g in ((0, 0), (0, 2), (2, 4), (6, 0))]


# ------------------------------------------------------------------------------------------------ forgeries
def _refuser(linked_airs, name, k=0):
    """-> (the shard's honest tables, refused(fn, ...)): the honest tables are accepted by the `_accepts` that then refuses
    each forgery"""
    canon, pubs, cycles, preps, words = _tables(name, k)
    ok = lambda c, pv, why, **kw: TC._accepts(linked_airs, c, preps, pv, cycles, words, why, **kw)
    why = {}
    assert ok(canon, pubs, why), (name, why)

    def refused(fn, air=None, bus=None, clean=(), pv=None, **kw):
        c = [t.copy() for t in canon]
        fn(c)
        why = {}
        assert not ok(c, pubs if pv is None else pv, why, **kw)
        names = {n for _r, n in why["air"].get(9, ())}
        if air is not None:
            assert air in names, (air, names)
        assert not names & set(clean), names
        if bus is not None:
            assert why["bus"].get(bus), (bus, list(why["bus"]))
        return why
    return canon, pubs, refused


def test_forged_journal_limbs_are_refused(linked_airs):
    canon, _pubs, refused = _refuser(linked_airs, "j14")
    io = canon[9]
    r = int(np.nonzero((io[:, Q_CW] == 1) & (io[:, Q_JH] == 1))[0][0])
    jl = int(io[r, Q_JL])
    # the same JPOS split another way: JL takes bit 14.  The AIR holds; 4 JL is no 16-bit value
    def resplit(c):
        c[9][r, Q_JL], c[9][r, Q_JH], c[9][r, Q_JL4] = jl + 16384, 0, 4 * (jl + 16384)
    why = refused(resplit, bus=BUS_RANGE16, clean=("jpos limbs", "jl4", "jpos"))
    assert (4 * (jl + 16384),) in why["bus"][BUS_RANGE16] and (jl + 16384,) in why["bus"][BUS_RANGE16] and 9 not in why["air"]
    # JH cut at bit 16, as a 16-bit limb would be
    def high16(c):
        c[9][r, Q_JH] = int(io[r, Q_JPOS]) >> 16
    assert io[r, Q_JPOS] >> 16 != io[r, Q_JH]
    refused(high16, air="jpos limbs")


def test_forged_carry_is_refused(linked_airs):
    canon, _pubs, refused = _refuser(linked_airs, "carry1")
    io = canon[9]
    h = int(np.nonzero(io[:, Q_READ] == 1)[0][0])
    assert io[h, Q_C] == 1 and io[h, Q_NH] == 1
    # C = 0 with the carry left in NL: N_INPUT is the same sum
    def no_carry(c):
        t = c[9]
        t[h, Q_C], t[h, Q_NL], t[h, Q_NH] = 0, io[h, Q_NL] + 16384, 0
        t[h, Q_NL4] = 4 * t[h, Q_NL]
    why = refused(no_carry, bus=BUS_RANGE16, clean=("left lo", "left hi", "n_input", "nl4", "carry"))
    assert (4 * (int(io[h, Q_NL]) + 16384),) in why["bus"][BUS_RANGE16] and 9 not in why["air"]
    # POS split the same way on a word row: PH would be -1
    w = int(np.nonzero(io[:, Q_WORD] == 1)[0][1])
    def pos_resplit(c):
        t = c[9]
        t[w, Q_PL], t[w, Q_PH] = io[w, Q_PL] + 16384, P - 1
        t[w, Q_PL4] = 4 * t[w, Q_PL]
    why = refused(pos_resplit, bus=BUS_RANGE16, clean=("pos limbs", "pl4", "pos"))
    assert (P - 1,) in why["bus"][BUS_RANGE16] and 9 not in why["air"]
    # C = 2 where the sum carries once
    def two(c):
        c[9][h, Q_C] = 2
    refused(two, air="left lo")


def test_forged_capacity_borrow_is_refused(linked_airs):
    canon, _pubs, refused = _refuser(linked_airs, "cap16")
    io = canon[9]
    h = int(np.nonzero(io[:, Q_READ] == 1)[0][0])
    assert io[h, Q_KF] == 1 and io[h, Q_FLO] == 0xFFFD and io[h, Q_FHI] == 0
    # KF = 0: F_LO = B_LO - GOT is negative, F_HI takes the borrow's place
    def no_borrow(c):
        c[9][h, Q_KF], c[9][h, Q_FLO], c[9][h, Q_FHI] = 0, (0xFFFD - 65536) % P, 1
    why = refused(no_borrow, bus=BUS_RANGE16, clean=("cap lo", "cap hi", "zc", "min"))
    assert (P - 3,) in why["bus"][BUS_RANGE16] and 9 not in why["air"]
    def dropped(c):
        c[9][h, Q_KF] = 0
    refused(dropped, air="cap lo")


def test_forged_commit_length_is_refused(linked_airs):
    """a1 and REM of rem16's COMMIT raised by 2^25: 128 B_HI is no 16-bit value.  The table has 2^15 rows, so the judge
    is the io AIR on the head row with the row after it (a slice's last row wraps and is not judged) and the 16-bit range
    of what the head sends to RANGE16 -- the honest head passes the same two"""
    io = _io("rem16")
    h = int(np.nonzero(io[:, Q_COMMIT] == 1)[0][0])
    assert io[h, Q_B_HI] == 1 and io[h, Q_BH7] == 128 and io[h + 1, Q_CW] == 1
    pv = _io_publics([io[h, Q_POS], 0, 0, 0, 0, 0, io[h, Q_JPOS], 0])        # the slice's first row is the head

    def judge(rows):
        t = rows[h:h + 2]
        bad = {n for r, n in T._named(linked_airs[9], linked_airs[9].check_trace(t, pv)) if r == 0}
        sent = [int(t[0, c]) for c, m in RC.IO_RANGE if t[0, m] == 1]
        return bad, [v for v in sent if not 0 <= v < 1 << 16]
    assert judge(io) == (set(), [])
    forged = io.copy()
    forged[h, Q_B_HI] += 1 << 9
    forged[h, Q_REM] += 1 << 25
    forged[h, Q_BH7] = 128 * forged[h, Q_B_HI]
    forged[h, rv32io.Q_RINV] = rv32io.rv32im._inv(forged[h:h + 1, Q_REM])[0]
    bad, over = judge(forged)
    assert not bad & {"bh7", "rem commit", "rinv", "z", "keep lo", "call"} and over == [128 * 513]
    assert bad <= {"rem bytes"}                                 # the countdown into the first commit-word row, unless that follows too
    forged[h, Q_BH7] = 128                                      # BH7 left in range: the constraint that ties it to B_HI
    assert "bh7" in judge(forged)[0]


def test_forged_journal_start_is_refused(linked_airs):
    """shard 1 of j14x with its journal positions lowered by 2^14 in the public values and the table: the chain check
    refuses the run, and the log the verifier is handed no longer fits the public values"""
    canon, pubs, refused = _refuser(linked_airs, "j14x", 1)
    log = RC.log_of_table(canon[9])
    pub0, pub1 = RC.publics_of(_tables("j14x", 0)[1][9]), RC.publics_of(pubs[9])
    assert RC.check_commit_chain([pub0, pub1]) == 16388
    cp = p3.from_mont(pubs[9][:RC.PUB_COMMIT_DIGEST]).astype(np.int64)
    cp[RC.PUB_JPOS_START] = (cp[RC.PUB_JPOS_START] - 16384) % P
    cp[RC.PUB_JPOS_END] = (cp[RC.PUB_JPOS_END] - 16384) % P
    pv = list(pubs)
    pv[9] = np.concatenate([p3.to_mont(cp), pubs[9][RC.PUB_COMMIT_DIGEST:]])
    def lowered(c):
        t = c[9]
        t[:, Q_JPOS] = (t[:, Q_JPOS] - 16384) % P
        cw = t[:, Q_CW] == 1
        t[cw, Q_JH] = (t[cw, Q_JH] - 1) % P
    why = refused(lowered, pv=pv, log=log, clean=("jpos", "jpos limbs", "jpos start", "jpos end"))
    assert why["log"] and 9 not in why["air"]
    with pytest.raises(ValueError, match="shard 1"):
        RC.check_commit_chain([pub0, RC.publics_of(pv[9])])
    # the honest table with a log whose second position has bit 14 cleared (no digest of it exists: the positions of a
    # journal ascend); the public values with the digest of a log that differs in one word
    other = log.copy()
    assert other[1, 0] == 16385
    other[1, 0] ^= 1 << 14
    why = refused(lambda c: None, log=other)
    assert why["log"]
    with pytest.raises(_lib.RkError):
        RC.log_root(other, 2)
    other = log.copy()
    other[1, 1] ^= 1
    pv = list(pubs)
    pv[9] = np.concatenate([pubs[9][:RC.PUB_COMMIT_DIGEST], RC.log_root(other, 2)])
    why = refused(lambda c: None, pv=pv, log=log)
    assert why["digest"] and not why["log"]
