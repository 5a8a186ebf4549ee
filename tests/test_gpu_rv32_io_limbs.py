"""The io and commit forms of the rv32im-mem chip set on the GPU where the io table's limbs carry (the guests of
tests/rv32_limb_programs.py; the CPU side is tests/test_rv32_io_limbs.py): the ten tables, the public values, the commit log
and the link journals of rk_exec_rv32commit_shard_device / rk_exec_rv32io_shard_device against numpy word for word, runs
proven and verified end to end with the journal cut from the logs, and the host's refusal of a shard whose tables would be
taller than twice the cpu table.

io_offsets_kernel scans one block per 128 ecalls: `mixed` (141 heads of three kinds) has a second block and its first
block's three totals -- rows, commit words, commit bytes -- differ pairwise.  io_rows_kernel runs one block per 128 io
rows: 256 blocks for rem16 and got14 (2^15 rows under a cpu table of 2^14), whose memop tables are as tall; under plain
io=True the kernel's other instantiation computes the padding's stream position as pos_start + total - count.  Every case
runs with 8 queries; every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import rv32_limb_programs as LL
from raiko_amd import executor as X
from raiko_amd import _lib, rv32commit, rv32elf, rv32io, rv32link, rv32_sets
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

FAST = dict(queries=8, pow_bits=6)
IO_LOGS = {"j14": [13], "j14x": [13, 2], "rem16": [15], "carry2": [14, 14], "carry1": [4], "got14": [15], "cap16": [3], "gap14": [3],
           "mixed": [9]}
_refs = {}


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


def _ref(name, blob, commit):
    """the run in numpy, linked, computed once: (the executor's run, [(tables, init, journal[, log])])"""
    if (name, commit) not in _refs:
        fn, words = LL.RUNS[name]
        elf = fn()
        ex = X.execute(elf, words, segment_limit_po2=LL.PO2[name], record_trace=True)
        _refs[name, commit] = ex, rv32_sets.shards("rv32im-mem", ex, rv32elf.program_image(elf), link=True, params=blob, io=True,
                                                   input_words=words, commit=commit)
    return _refs[name, commit]


def _compare(hal, blob, name, link, commit):
    fn, words = LL.RUNS[name]
    elf = fn()
    ref_ex, ref = _ref(name, blob, commit)
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", link=link, io=True, commit=commit)
    try:
        out = X.execute_rv32_device(hal, elf, words, LL.PO2[name], chips="rv32im-mem", key=key, link=link, io=True, commit=commit)
        ex, shards, _dev, bufs = out[:4]
        try:
            hal.sync()
            assert len(shards) == len(ref) == LL.SHARDS[name] and ex.journal == ref_ex.journal == LL.expected_journal(name)
            assert (ex.exit_code, ex.input_words_read) == LL.EXPECT[name]
            for k, (r, d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
                assert len(tables) == 10 and np.array_equal(init, r[1])
                for i, (rt, (b, lg), t) in enumerate(zip(r[0], d, tables)):
                    assert lg == rt.log_height and np.array_equal(b.to_host(), rt.trace.reshape(-1)), (name, k, i)
                    if i == rv32link.MEMORY_TABLE and not link:         # the reference is the linked one: its digest
                        assert np.asarray(t.public_values).size == 0
                    else:
                        assert np.array_equal(t.public_values, rt.public_values), (name, k, i)
                assert tables[rv32io.IO_TABLE].public_values.size == (24 if commit else 14)
                if link:
                    assert np.array_equal(out[4][k], r[2])
                if commit:
                    assert out[-1][k].dtype == np.uint32 and np.array_equal(out[-1][k], r[-1]), (name, k)
            assert [t[rv32io.IO_TABLE].log_height for t, _i in shards] == IO_LOGS[name]
        finally:
            _free(bufs)
    finally:
        key.close()


CASES = [(name, link) for name in sorted(LL.RUNS) for link in ((False, True) if name in ("j14x", "carry2", "mixed") else (True,))]


@pytest.mark.parametrize("name,link", CASES)
def test_commit_form_tables_publics_and_log_equal_numpy(hal, blob, name, link):
    _compare(hal, blob, name, link, commit=True)


@pytest.mark.parametrize("name", LL.READ_ONLY)
def test_io_form_tables_and_publics_equal_numpy(hal, blob, name):
    _compare(hal, blob, name, link=True, commit=False)


def _prove(blob, name):
    fn, words = LL.RUNS[name]
    elf = fn()
    want = LL.expected_journal(name)
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=LL.PO2[name], params=blob, chips="rv32im-mem", link=True, io=True,
                                                commit=True)
    assert len(proofs) == LL.SHARDS[name] and ex.journal == want
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height, journals=ex.journals, image=rv32link.memory_image(elf))
    got = X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc, **vk, input_words=words,
                                  commit_logs=ex.commit_logs, expected_journal=want)
    assert got == LL.EXPECT[name] + (want,)
    assert [t[rv32io.IO_TABLE].log_height for t, _i in shards] == IO_LOGS[name]
    return ex, shards, proofs, vk, words


@pytest.mark.parametrize("name", ["carry2", "cap16", "gap14", "mixed", "rem16"])
def test_proven_and_verified_end_to_end(blob, name):
    _prove(blob, name)


def test_j14x_end_to_end_and_a_log_with_bit_14_cleared(blob):
    ex, shards, proofs, vk, words = _prove(blob, "j14x")
    assert [len(log) for log in ex.commit_logs] == [4096, 2] and ex.commit_logs[1][:, 0].tolist() == [16383, 16385]
    bad = [log.copy() for log in ex.commit_logs]
    bad[1][1, 0] ^= 1 << 14
    with pytest.raises(ValueError, match=r"shard 1: the proof does not verify \(reason 2\)"):
        X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words, commit_logs=bad)
    # ... and as claims under the proof itself: the tuple the table sent holds JH = 1
    tables, init, *_ = shards[1]
    from raiko_amd import p3
    vt = X.rv32_verifier_tables(tables, proofs[1], prep_root=ex.prep_root, program_log_height=ex.program_log_height)
    claims = rv32link.claims_of(ex.journals[1])                # the shard reads no input: no claims on BUS_INPUT
    assert p3.verify(vt, proofs[1], init, blob, prep_root=ex.prep_root, claims=claims + rv32commit.claims_of(ex.commit_logs[1])) == 0
    assert p3.verify(vt, proofs[1], init, blob, prep_root=ex.prep_root, claims=claims + rv32commit.claims_of(bad[1])) == 8


def test_shards_too_tall_are_refused_on_the_host(hal, blob):
    """a READ of 20000 words and a COMMIT of 70000 bytes in a shard of 2^13 cycles: the sizes calls refuse, so nothing is
    allocated or launched; the context then writes carry1's tables as before"""
    lib = _lib.load()
    refusing = {"read": ("rk_exec_rv32io_sizes", "rk_exec_rv32commit_sizes"), "commit": ("rk_exec_rv32commit_sizes",)}
    for name, (fn, words) in LL.REFUSED.items():
        elf = fn()
        st = X.Stepper(elf, words, 13)
        try:
            seg = st.step()
            assert seg.po2 == 13
            mo, bd, io = C.c_size_t(7), C.c_size_t(7), C.c_size_t(7)
            for entry in refusing[name]:
                assert getattr(lib, entry)(st._h, 0, C.byref(mo), C.byref(bd), C.byref(io)) == _lib.RK_ERR_CAPACITY, (name, entry)
            if name == "read":
                assert lib.rk_exec_rv32mem_sizes(st._h, 0, C.byref(mo), C.byref(bd)) == _lib.RK_ERR_CAPACITY
            else:                                               # the io form does not read a COMMIT's words: two heads
                _lib.check(None, lib.rk_exec_rv32io_sizes(st._h, 0, C.byref(mo), C.byref(bd), C.byref(io)))
                assert io.value == 2
        finally:
            st.close()
        for commit in ((False, True) if name == "read" else (True,)):
            key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", link=True, io=True, commit=commit)
            try:
                with pytest.raises(_lib.RkError) as e:
                    X.execute_rv32_device(hal, elf, words, 13, chips="rv32im-mem", key=key, link=True, io=True, commit=commit)
                assert e.value.status == _lib.RK_ERR_CAPACITY
            finally:
                key.close()
    _compare(hal, blob, "carry1", link=True, commit=True)


def test_the_pipeline_refuses_shards_too_tall_and_goes_on(blob):
    pipe = X.P3Pipeline(blob, chips="rv32im-mem", link=True, io=True, commit=True)
    try:
        for name, (fn, words) in LL.REFUSED.items():
            with pytest.raises(_lib.RkError) as e:
                pipe.run(fn(), words, shard_po2=13)
            assert e.value.status == _lib.RK_ERR_CAPACITY, name
        fn, words = LL.RUNS["carry1"]
        ex, proofs, _kept = pipe.run(fn(), words, shard_po2=13)
    finally:
        pipe.close()
    assert len(proofs) == 1 and (ex.exit_code, ex.input_words_read) == LL.EXPECT["carry1"] and ex.journal == b""
