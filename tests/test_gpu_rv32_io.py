"""The io form of the rv32im-mem chip set on the GPU (raiko_amd/rv32io.py): rk_rv32io_prep_device's key and the ten tables
of rk_exec_rv32io_shard_device against numpy word for word, with and without the link; runs end to end through the shard
pool with the input claims and through the pipeline, checked by verify_rv32_execution(input_words=); proofs refused for a
foreign input (reason 2), for other claims under a consistent digest (reason 8) and under the other form's root; the run
fed other words than the verifier's input, which link=True accepts and io=True refuses; io=False unchanged; one run
under risc0's parameter set.

io_rows_kernel runs one block of min(rows, 128) lanes per 128 io rows; io_offsets_kernel one block per 128 ecalls, whose
totals mscan_kernel scans (its chunks are nb * t / 1024: one block is one chunk, a second block is the first size at which
a chunk's offset comes from another lane's sum).  Sizes where another path is taken: `halt` 2 rows (a block of two lanes);
`big125` 128 rows (the tallest one-block table); `big200` 256 rows (a second block; the READ's head lies in block 0 and
its words in both); `many` 131 ecalls (a second block of io_offsets_kernel and mscan_kernel's second chunk: 129 is the
first such count).  Every case runs at po2 = 13 with 8 queries; every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import rv32_io_programs as IP
import rv32_link_programs as LP
from raiko_amd import executor as X
from raiko_amd import _lib, p3, rv32elf, rv32io, rv32link, rv32_sets
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
    fn, words = IP.RUNS[name]
    elf = fn()
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", link=link, io=True)
    try:
        ref_ex = X.execute(elf, words, segment_limit_po2=13, record_trace=True)
        ref = rv32_sets.shards("rv32im-mem", ref_ex, rv32elf.program_image(elf), airs=key.airs, link=link, params=blob, io=True,
                               input_words=words)
        # the key: the device's preprocessed matrices commit to the root the numpy matrices give
        host_key = p3.setup(hal, ref[0][0])
        try:
            assert np.array_equal(host_key.root, key.root)
        finally:
            host_key.close()
        out = X.execute_rv32_device(hal, elf, words, 13, chips="rv32im-mem", key=key, link=link, io=True)
        ex, shards, _dev, bufs = out[:4]
        try:
            hal.sync()
            assert len(shards) == len(ref) and (ex.exit_code, ex.input_words_read) == (ref_ex.exit_code, ref_ex.input_words_read)
            for k, (r, d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
                assert len(tables) == 10 and np.array_equal(init, r[1])
                for i, (rt, (b, lg), t) in enumerate(zip(r[0], d, tables)):
                    assert lg == rt.log_height and np.array_equal(b.to_host(), rt.trace.reshape(-1)), (name, k, i)
                    assert np.array_equal(t.public_values, rt.public_values), (name, k, i)
                if link:
                    assert np.array_equal(out[4][k], r[2])
        finally:
            _free(bufs)
        return [r[0][rv32io.IO_TABLE].log_height for r in ref]
    finally:
        key.close()


@pytest.mark.parametrize("name", sorted(IP.RUNS))
def test_ten_tables_equal_numpy(hal, blob, name):
    logs = _compare(hal, blob, name, link=name in ("reads", "three"))
    want = {"halt": [1], "big125": [7], "big200": [8], "many": [8], "three": [2, 1, 3]}
    if name in want:
        assert logs == want[name]


def test_refused_before_any_launch(hal, blob):
    """NULL buffers, an io table that is no power of two >= 2, below what rk_exec_rv32io_sizes gives or above 2^(po2 + 1)"""
    fn, words = IP.RUNS["reads"]
    elf = fn()
    lib = _lib.load()
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", io=True)
    st = X.Stepper(elf, words, 13)
    try:
        seg = st.step()
        mo, bd, io = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32io_sizes(st._h, 0, C.byref(mo), C.byref(bd), C.byref(io)))
        assert io.value == 16 and lib.rk_exec_rv32io_sizes(st._h, 0, C.byref(mo), C.byref(bd), None) == _lib.RK_ERR_INVALID
        md = C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32im_sizes(st._h, 0, C.byref(md)))
        rows = [1 << seg.po2, 1 << key.program_log_height, 32, 1 << 18, 1 << 16, 1 << 12, md.value, mo.value, bd.value, 2 << seg.po2]
        bufs = [hal.alloc_elem(a.width * r) for a, r in zip(key.airs, rows)]
        try:
            for b in bufs:
                b.copy_from(np.full(b.words, 7, dtype=np.uint32))
            pubs = np.zeros(14, dtype=np.uint32)
            up = lambda a: a.ctypes.data_as(_lib.u32p)

            def call(io_rows, d_io=bufs[9], h_pubs=pubs):
                p = [C.c_void_p(b.ptr) for b in bufs]
                return lib.rk_exec_rv32io_shard_device(hal._ctx, st._h, 0, up(key.seg_vaddr), up(key.seg_words), key.seg_vaddr.size,
                                                       C.c_void_p(key.d_words.ptr), p[0], p[1], rows[1], p[2], p[3], p[4], p[5], p[6], rows[6],
                                                       p[7], rows[7], p[8], rows[8], None if d_io is None else C.c_void_p(d_io.ptr), io_rows,
                                                       None if h_pubs is None else up(h_pubs))
            for r in (0, 1, 3, 24, 4 << seg.po2):
                assert call(r) == _lib.RK_ERR_INVALID, r
            assert call(8) == _lib.RK_ERR_CAPACITY
            assert call(16, d_io=None) == _lib.RK_ERR_INVALID and call(16, h_pubs=None) == _lib.RK_ERR_INVALID
            hal.sync()
            assert all((b.to_host() == 7).all() for b in bufs) and not pubs.any()
            assert call(32) == 0                               # a taller table than the segment needs: its own digest
            hal.sync()
            got = rv32io.publics_of(pubs)
            assert (got["pos_start"], got["pos_end"], got["n_input"], got["halted"], got["exit"]) == (0, 6, 6, 1, 5)
            assert np.array_equal(got["digest"], rv32io.stream_root(0, words, 5, blob))
        finally:
            for b in bufs:
                b.free()
    finally:
        st.close()
        key.close()


@pytest.mark.parametrize("link", [False, True])
def test_three_shards_end_to_end(blob, link):
    fn, words = IP.RUNS["three"]
    elf = fn()
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, batch=2, chips="rv32im-mem", link=link, io=True)
    assert len(proofs) == 3 and (ex.exit_code, ex.input_words_read) == (9, 5)
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height)
    if link:
        vk.update(journals=ex.journals, image=rv32link.memory_image(elf))
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc, **vk, input_words=words) == (9, 5)
    with pytest.raises(ValueError, match="shard 0"):
        X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words + [1])            # N_INPUT is not the input's length
    other = list(words)
    other[3] ^= 1                                                                               # a word shard 2 reads
    with pytest.raises(ValueError, match=r"shard 2: the proof does not verify \(reason 2\)"):
        X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=other)
    if link:
        return
    # the pipeline proves the same statements
    ex2, pproofs, _kept = X.execute_and_prove_p3_pipelined(elf, words, shard_po2=13, params=blob, chips="rv32im-mem", io=True)
    assert all(np.array_equal(a, b) for a, b in zip(proofs, pproofs)) and (ex2.exit_code, ex2.input_words_read) == (9, 5)
    # shard 2 alone: its slice; other claims under the consistent digest; no claims; shard 0's statement
    tables, init = shards[2]
    pf, kv = proofs[2], dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height)
    assert X.verify_rv32_shard(tables, pf, init, blob, **kv, input_words=words) == 0
    vt = X.rv32_verifier_tables(tables, pf, **kv)
    assert p3.verify(vt, pf, init, blob, prep_root=ex.prep_root, claims=rv32io.claims_of(2, words[2:5])) == 0
    assert p3.verify(vt, pf, init, blob, prep_root=ex.prep_root, claims=rv32io.claims_of(2, other[2:5])) == 8
    assert p3.verify(vt, pf, init, blob, prep_root=ex.prep_root, claims=rv32io.claims_of(1, words[1:4])) == 8
    assert p3.verify(vt, pf, init, blob, prep_root=ex.prep_root) == 8
    # POS_START of shard 1 is not POS_END of shard 0: shards 0 and 2 without the one between them chain on pc alone
    pubs = [rv32io.publics_of(t[rv32io.IO_TABLE].public_values) for t, _i in shards]
    bad = [dict(p) for p in pubs]
    bad[1]["pos_start"] = bad[1]["pos_end"] = 3
    with pytest.raises(ValueError, match="shard 1"):
        rv32io.check_io_chain(bad, words)


def test_the_two_forms_have_two_keys(hal, blob):
    """an io proof against the plain rv32im-mem root, and the reverse"""
    fn, words = IP.RUNS["short"]
    elf = fn()
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, chips="rv32im-mem", io=True)
    mex, mshards, mproofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, chips="rv32im-mem")
    assert not np.array_equal(ex.prep_root, mex.prep_root) and ex.program_log_height == mex.program_log_height
    assert (ex.exit_code, ex.input_words_read) == (0x12345678, 6)
    plh = ex.program_log_height
    (tables, init), (mtables, minit) = shards[0], mshards[0]
    assert X.verify_rv32_shard(tables, proofs[0], init, blob, ex.prep_root, plh, input_words=words) == 0
    assert X.verify_rv32_shard(tables, proofs[0], init, blob, mex.prep_root, plh, input_words=words) != 0
    assert X.verify_rv32_shard(mtables, mproofs[0], minit, blob, mex.prep_root, plh) == 0
    assert X.verify_rv32_shard(mtables, mproofs[0], minit, blob, ex.prep_root, plh) != 0


def test_the_hole_is_closed(blob):
    """a prover runs the guest on words of their own.  Under link=True the run proves and verifies: nothing names the
    input.  Under io=True the same run, proven, is refused by the verifier who holds the real input"""
    fn, words = IP.RUNS["reads"]
    elf = fn()
    theirs = [w ^ 0x5A5A5A5A for w in words]
    lex, lshards, lproofs = X.execute_and_prove_p3(elf, theirs, shard_po2=13, params=blob, chips="rv32im-mem", link=True)
    assert X.verify_rv32_execution(lshards, lproofs, blob, prep_root=lex.prep_root, program_log_height=lex.program_log_height,
                                   journals=lex.journals, image=rv32link.memory_image(elf)) is True
    ex, shards, proofs = X.execute_and_prove_p3(elf, theirs, shard_po2=13, params=blob, chips="rv32im-mem", link=True, io=True)
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height, journals=ex.journals, image=rv32link.memory_image(elf))
    assert X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=theirs) == (5, 6)
    with pytest.raises(ValueError, match=r"shard 0: the proof does not verify \(reason 2\)"):
        X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words)


def test_io_false_is_unchanged(hal, blob):
    fn, words = IP.RUNS["reads"]
    elf = fn()
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem")
    try:
        ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, words, 13, chips="rv32im-mem", key=key)
        try:
            hal.sync()
            ref_ex = X.execute(elf, words, segment_limit_po2=13, record_trace=True)
            ref = X.p3_rv32mem_shards(ref_ex, rv32elf.program_image(elf), airs=key.airs)
            for (rt, _ri), d, (tables, _init) in zip(ref, bufs, shards):
                assert len(tables) == 9
                for r, (b, lg) in zip(rt, d):
                    assert lg == r.log_height and np.array_equal(b.to_host(), r.trace.reshape(-1))
        finally:
            _free(bufs)
    finally:
        key.close()
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, chips="rv32im-mem")
    assert X.verify_rv32_execution(shards, proofs, blob, prep_root=ex.prep_root, program_log_height=ex.program_log_height) is True


def test_under_risc0s_parameter_set():
    preset, over = LP.LINK_SETS["risc0"]
    blob = H.make_params(preset, **over)
    fn, words = IP.RUNS["reads"]
    elf = fn()
    ex, shards, proofs = X.execute_and_prove_p3(elf, words, shard_po2=13, params=blob, chips="rv32im-mem", link=True, io=True)
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height, journals=ex.journals, image=rv32link.memory_image(elf))
    assert X.verify_rv32_execution(shards, proofs, blob, **vk, input_words=words) == (5, 6)
    pub = rv32io.publics_of(shards[0][0][rv32io.IO_TABLE].public_values)
    assert np.array_equal(pub["digest"], rv32io.stream_root(0, words, shards[0][0][rv32io.IO_TABLE].log_height, blob))
    assert not np.array_equal(pub["digest"], rv32io.stream_root(0, words, shards[0][0][rv32io.IO_TABLE].log_height))
