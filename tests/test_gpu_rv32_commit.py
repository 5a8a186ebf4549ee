"""The commit form of the rv32im-mem chip set on the GPU (raiko_amd/rv32commit.py): the ten tables, the io public values
and the commit log of rk_exec_rv32commit_shard_device against numpy word for word, with and without the link; the
refusals before any launch; a three-shard run end to end through the pipeline and the shard pool, the verifier's journal
the executor's; a journal forged by one byte, which io=True accepts and commit=True refuses; commit=False unchanged; one
run under risc0's parameter set.

io_rows_kernel runs one block of min(rows, 128) lanes per 128 io rows; io_offsets_kernel one block per 128 ecalls, whose
three totals mscan_kernel scans.  Sizes where another path is taken: `three` shard 1, an io table of 2 padding rows; `big`
256 rows (a COMMIT's head in block 0, its 129 commit-word rows in both blocks); `many` 131 ecalls (a second block of
io_offsets_kernel: dense indices and journal positions that come from mscan_kernel's second chunk).  Every case runs at
po2 = 13 with 8 queries; every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import rv32_commit_programs as CP
import rv32_link_programs as LP
from raiko_amd import executor as X
from raiko_amd import _lib, rv32commit, rv32elf, rv32io, rv32link, rv32_sets
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

FAST = dict(queries=8, pow_bits=6)


@pytest.fixture(scope="module")
def hal():
    h = H.HipHal(0)
    h.set_params(1, **FAST)
    yield h
    h.close()


@pytest.fixture(scope="module")
def blob():
    return H.make_params(1, **FAST)


def _free(bufs):
    for d in bufs:
        for b, _lg in d:
            b.free()


def _compare(hal, blob, name, link):
    fn, words = CP.RUNS[name]
    elf = fn()
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", link=link, io=True, commit=True)
    try:
        ref_ex = X.execute(elf, words, segment_limit_po2=13, record_trace=True)
        ref = rv32_sets.shards("rv32im-mem", ref_ex, rv32elf.program_image(elf), airs=key.airs, link=link, params=blob, io=True,
                               input_words=words, commit=True)
        out = X.execute_rv32_device(hal, elf, words, 13, chips="rv32im-mem", key=key, link=link, io=True, commit=True)
        ex, shards, _dev, bufs = out[:4]
        try:
            hal.sync()
            assert len(shards) == len(ref) and ex.journal == ref_ex.journal == CP.expected_journal(name)
            for k, (r, d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
                assert len(tables) == 10 and np.array_equal(init, r[1])
                for i, (rt, (b, lg), t) in enumerate(zip(r[0], d, tables)):
                    assert lg == rt.log_height and np.array_equal(b.to_host(), rt.trace.reshape(-1)), (name, k, i)
                    assert np.array_equal(t.public_values, rt.public_values), (name, k, i)
                assert tables[rv32io.IO_TABLE].public_values.size == 24
                if link:
                    assert np.array_equal(out[4][k], r[2])
                assert out[-1][k].dtype == np.uint32 and np.array_equal(out[-1][k], r[-1]), (name, k)
        finally:
            _free(bufs)
        return [r[0][rv32io.IO_TABLE].log_height for r in ref]
    finally:
        key.close()


@pytest.mark.parametrize("link", [False, True])
@pytest.mark.parametrize("name", sorted(CP.RUNS))
def test_ten_tables_publics_and_log_equal_numpy(hal, blob, name, link):
    logs = _compare(hal, blob, name, link)
    want = {"three": [2, 1, 2], "big": [8], "many": [9], "small": [5]}
    if name in want:
        assert logs == want[name]


def test_refused_before_any_launch(hal, blob):
    """NULL buffers, no log, an io table that is no power of two >= 2, below what rk_exec_rv32commit_sizes gives or above
    2^(po2 + 1), a memop table sized for the access list without the commit reads"""
    fn, words = CP.RUNS["small"]
    elf = fn()
    lib = _lib.load()
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", io=True, commit=True)
    st = X.Stepper(elf, words, 13)
    try:
        seg = st.step()
        mo, bd, io = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32commit_sizes(st._h, 0, C.byref(mo), C.byref(bd), C.byref(io)))
        assert (mo.value, io.value) == (16, 32) and lib.rk_exec_rv32commit_sizes(st._h, 0, C.byref(mo), C.byref(bd), None) == _lib.RK_ERR_INVALID
        mo_io, bd_io, io_io = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32io_sizes(st._h, 0, C.byref(mo_io), C.byref(bd_io), C.byref(io_io)))
        assert (mo_io.value, io_io.value) == (2, 16)            # the io form's sizes: the access list alone
        md = C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32im_sizes(st._h, 0, C.byref(md)))
        rows = [1 << seg.po2, 1 << key.program_log_height, 32, 1 << 18, 1 << 16, 1 << 12, md.value, mo.value, bd.value, 2 << seg.po2]
        bufs = [hal.alloc_elem(a.width * r) for a, r in zip(key.airs, rows)]
        d_log = hal.alloc_elem(3 * rows[9])
        try:
            for b in bufs + [d_log]:
                b.copy_from(np.full(b.words, 7, dtype=np.uint32))
            pubs = np.zeros(24, dtype=np.uint32)
            n_log = C.c_size_t(99)
            up = lambda a: a.ctypes.data_as(_lib.u32p)

            def call(io_rows, d_io=bufs[9], h_pubs=pubs, log=d_log, n=n_log, memop_rows=rows[7]):
                p = [C.c_void_p(b.ptr) for b in bufs]
                return lib.rk_exec_rv32commit_shard_device(
                    hal._ctx, st._h, 0, up(key.seg_vaddr), up(key.seg_words), key.seg_vaddr.size, C.c_void_p(key.d_words.ptr), p[0], p[1],
                    rows[1], p[2], p[3], p[4], p[5], p[6], rows[6], p[7], memop_rows, p[8], rows[8],
                    None if d_io is None else C.c_void_p(d_io.ptr), io_rows, None if h_pubs is None else up(h_pubs),
                    None if log is None else C.c_void_p(log.ptr), None if n is None else C.byref(n))
            for r in (0, 1, 3, 24, 4 << seg.po2):
                assert call(r) == _lib.RK_ERR_INVALID, r
            assert call(16) == _lib.RK_ERR_CAPACITY
            assert call(32, d_io=None) == _lib.RK_ERR_INVALID and call(32, h_pubs=None) == _lib.RK_ERR_INVALID
            assert call(32, log=None) == _lib.RK_ERR_INVALID and call(32, n=None) == _lib.RK_ERR_INVALID
            assert call(32, memop_rows=mo_io.value) == _lib.RK_ERR_INVALID
            hal.sync()
            assert all((b.to_host() == 7).all() for b in bufs + [d_log]) and not pubs.any() and n_log.value == 99
            assert call(64) == 0                               # a taller table than the segment needs: its own digest
            hal.sync()
            got = rv32commit.publics_of(pubs)
            want = CP.expected_journal("small")
            assert (got["jpos_start"], got["jpos_end"], got["halted"], got["exit"], n_log.value) == (0, len(want), 1, 5, 12)
            log = d_log.to_host().reshape(-1, 3)[:12]
            assert np.array_equal(got["commit_digest"], rv32commit.log_root(log, 6, blob)) and rv32commit.log_bytes(got, log) == want
        finally:
            for b in bufs + [d_log]:
                b.free()
    finally:
        st.close()
        key.close()


def test_three_shards_end_to_end_through_the_pipeline(blob):
    fn, words = CP.RUNS["three"]
    elf = fn()
    want = CP.expected_journal("three")
    pipe = X.P3Pipeline(blob, chips="rv32im-mem", link=True, io=True, commit=True)
    try:
        ex, proofs, kept = pipe.run(elf, words, shard_po2=13, keep_tables=True)
    finally:
        pipe.close()
    assert len(proofs) == 3 and ex.journal == want and ex.exit_code == 9 and len(ex.commit_logs) == 3
    assert [len(log) for log in ex.commit_logs] == [2, 0, 2]
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height, journals=ex.journals, image=rv32link.memory_image(elf))
    got = X.verify_rv32_execution(kept, proofs, blob, entry_pc=ex.segments[0].start_pc, **vk, input_words=words,
                                  commit_logs=ex.commit_logs, expected_journal=want)
    assert got == (9, 0, want)
    # the shard pool proves the same statements
    ex2, shards, proofs2 = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, batch=2, chips="rv32im-mem", link=True, io=True,
                                                  commit=True)
    assert all(np.array_equal(a, b) for a, b in zip(proofs, proofs2)) and ex2.journal == want
    assert all(np.array_equal(a, b) for a, b in zip(ex.commit_logs, ex2.commit_logs))
    # a log with one byte changed: reason 2 before the proof is read; a log whose digest is kept but whose claims differ
    # cannot be made by the verifier's side alone, so the proof is checked against a foreign log of the same shape
    bad = [log.copy() for log in ex.commit_logs]
    bad[2][0, 1] ^= 0x100
    with pytest.raises(ValueError, match=r"shard 2: the proof does not verify \(reason 2\)"):
        X.verify_rv32_execution(kept, proofs, blob, **vk, input_words=words, commit_logs=bad)
    tables, init = kept[2]
    kv = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height)
    vt = X.rv32_verifier_tables(tables, proofs[2], **kv)
    from raiko_amd import p3
    link_claims = rv32link.claims_of(ex.journals[2])
    assert p3.verify(vt, proofs[2], init, blob, prep_root=ex.prep_root, claims=link_claims + rv32commit.claims_of(ex.commit_logs[2])) == 0
    assert p3.verify(vt, proofs[2], init, blob, prep_root=ex.prep_root, claims=link_claims + rv32commit.claims_of(bad[2])) == 8
    assert p3.verify(vt, proofs[2], init, blob, prep_root=ex.prep_root, claims=link_claims) == 8
    with pytest.raises(ValueError, match="the proven journal"):
        X.verify_rv32_execution(kept, proofs, blob, **vk, input_words=words, commit_logs=ex.commit_logs, expected_journal=want[:-1] + b"\0")


def test_the_hole_is_closed(blob):
    """a prover hands over a journal that differs in one byte.  Under io=True, link=True the run verifies whatever the
    journal: nothing in the statement names it.  Under commit=True the verifier cuts the journal from the logs the proofs
    are bound to, and the forged one is refused"""
    fn, words = CP.RUNS["read"]
    elf = fn()
    want = CP.expected_journal("read")
    forged = bytes([want[0] ^ 1]) + want[1:]
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, chips="rv32im-mem", link=True, io=True)
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height, journals=ex.journals, image=rv32link.memory_image(elf))
    ex.journal = forged
    assert X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words) == (2, 4)      # and ex.journal is anything
    with pytest.raises(ValueError, match="expected_journal goes with commit_logs"):
        X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words, expected_journal=forged)
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, chips="rv32im-mem", link=True, io=True, commit=True)
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height, journals=ex.journals, image=rv32link.memory_image(elf))
    assert X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words, commit_logs=ex.commit_logs,
                                   expected_journal=want) == (2, 4, want)
    with pytest.raises(ValueError, match="the proven journal"):
        X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words, commit_logs=ex.commit_logs, expected_journal=forged)
    with pytest.raises(ValueError):
        X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words)                   # 24 public values go with a log


def test_commit_false_is_unchanged(hal, blob):
    """the io form's instantiations of the kernels the commit form shares with it write the io form's tables"""
    fn, words = CP.RUNS["read"]
    elf = fn()
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", io=True)
    try:
        ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, words, 13, chips="rv32im-mem", key=key, io=True)
        try:
            hal.sync()
            ref_ex = X.execute(elf, words, segment_limit_po2=13, record_trace=True)
            ref = rv32_sets.shards("rv32im-mem", ref_ex, rv32elf.program_image(elf), airs=key.airs, params=blob, io=True, input_words=words)
            for (rt, _ri), d, (tables, _init) in zip(ref, bufs, shards):
                assert len(tables) == 10 and tables[9].public_values.size == 14 and [t.air.width for t in tables][7::2] == [64, 47]
                for r, (b, lg), t in zip(rt, d, tables):
                    assert lg == r.log_height and np.array_equal(b.to_host(), r.trace.reshape(-1))
                    assert np.array_equal(t.public_values, r.public_values)
        finally:
            _free(bufs)
    finally:
        key.close()


def test_under_risc0s_parameter_set():
    preset, over = LP.LINK_SETS["risc0"]
    blob = H.make_params(preset, **over)
    fn, words = CP.RUNS["small"]
    elf = fn()
    want = CP.expected_journal("small")
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, chips="rv32im-mem", link=True, io=True, commit=True)
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height, journals=ex.journals, image=rv32link.memory_image(elf))
    assert X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words, commit_logs=ex.commit_logs) == (5, 0, want)
    io = shards[0][0][rv32io.IO_TABLE]
    pub = rv32commit.publics_of(io.public_values)
    assert np.array_equal(pub["commit_digest"], rv32commit.log_root(ex.commit_logs[0], io.log_height, blob))
    assert not np.array_equal(pub["commit_digest"], rv32commit.log_root(ex.commit_logs[0], io.log_height))
