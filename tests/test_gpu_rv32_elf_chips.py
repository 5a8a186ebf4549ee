"""The rv32im-elf chip set on the GPU: rk_rv32elf_prep_device's four preprocessed matrices and
rk_exec_rv32elf_shard_device's seven traces against raiko_amd/rv32elf.py's numpy, word for word; wrong sizes refused
before any launch; a guest that rewrites its code refused; the public entry points (execute_and_prove_p3 and the
pipeline) under both parameter presets, every shard checked against the one root and chained; and THE BINDING: proofs of
one ELF are refused against the root of an ELF that differs in one immediate.

The exact integer reference (tests/p3_ref_prep.py) is too slow for the 2^18-row byte table, and the table is not shrunk
to suit it.  The large-table proofs are held by four things instead: the device tables are the numpy tables (here), the
numpy tables satisfy every AIR and balance every bus (tests/test_rv32_elf_chips.py, Air.check_trace), the pool's proofs
are the single-context rk_p3_prove_key's words (tests/test_gpu_p3_shards_key.py, where that path is held to the exact
reference at small shapes; and here, against proofs made from the numpy tables), and the keyed verifier accepts them."""
import ctypes as C

import numpy as np
import pytest

import rv32_elf_programs as EP
import rv32_m_programs as MP
from raiko_amd import _lib, p3, rv32elf
from raiko_amd import executor as X
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

INPUT = [11, 22, 33, 44]
FAST = dict(queries=8, pow_bits=6)
PROGRAMS = {"m1": lambda: MP.m_program(1), "m25": lambda: MP.m_program(25), "mixed": lambda: MP.mixed_program(400),
            "second": EP.second_segment_program, "pow2": EP.pow2_program}


@pytest.fixture(scope="module")
def hal():
    h = H.HipHal(0)
    h.set_params(1, **FAST)
    yield h
    h.close()


def free(bufs):
    for d in bufs:
        for b, _ in d:
            b.free()


def _prep_device(hal, elf, fill=None):
    """rk_rv32elf_prep_device into fresh buffers -> (status, the four matrices read back)"""
    lib = _lib.load()
    vaddr, count, words = X.program_image_c(elf)
    rows = 2
    while rows < words.size:
        rows <<= 1
    sizes = [rows * 42, 4 << 18, 1 << 16, 4 << 12]
    bufs = [hal.alloc_elem(s) for s in sizes]
    try:
        ptr = lambda a: a.ctypes.data_as(_lib.u32p)
        st = lib.rk_rv32elf_prep_device(hal._ctx, ptr(vaddr), ptr(count), vaddr.size, ptr(words), words.size, C.c_void_p(bufs[0].ptr),
                                        rows, *[C.c_void_p(b.ptr) for b in bufs[1:]])
        hal.sync()
        return st, [b.to_host() for b in bufs]
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("name,po2", [("m1", 13), ("m25", 13), ("mixed", 13), ("mixed", 16), ("second", 13), ("pow2", 13)])
def test_device_tables_equal_numpy(hal, name, po2):
    elf = PROGRAMS[name]()
    image = rv32elf.program_image(elf)
    want_prep = [p3.to_mont(m) for m in rv32elf.prep_tables(image)]
    st, got_prep = _prep_device(hal, elf)
    assert st == 0
    for i, (g, w) in enumerate(zip(got_prep, want_prep)):
        bad = np.nonzero(g.reshape(w.shape) != w)
        assert bad[0].size == 0, "preprocessed matrix %d: first difference at row %d col %d" % (i, bad[0][0], bad[1][0])
    key = X.setup_rv32_elf(hal, elf)
    try:
        assert key.program_log_height == want_prep[0].shape[0].bit_length() - 1 and key.root is not None
        ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, po2, chips="rv32im-elf", key=key)
        try:
            hal.sync()
            ref_ex = X.execute(elf, INPUT, segment_limit_po2=po2, record_trace=True)
            ref = X.p3_rv32elf_shards(ref_ex, image, airs=key.airs)
            assert len(ref) == len(shards) == len(bufs)
            if name == "m25":
                assert len(ref) >= 3 and ref_ex.segments[-1].cycles < 1 << po2
            for k, ((rt, rinit), d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
                assert np.array_equal(init, rinit) and len(d) == 7
                for i, (r, (b, lg), t) in enumerate(zip(rt, d, tables)):
                    g = b.to_host().reshape(1 << lg, t.air.width)
                    assert g.shape == r.trace.shape, (k, i)
                    bad = np.nonzero(g != r.trace)
                    assert bad[0].size == 0, "shard %d table %d: first difference at row %d col %d" % (k, i, bad[0][0], bad[1][0])
                    assert np.array_equal(t.public_values, r.public_values)
            if name == "second":    # rows of the second executable segment were counted
                n0 = image[0][1].size
                assert p3.from_mont(bufs[0][1][0].to_host())[n0:].any()
        finally:
            free(bufs)
    finally:
        key.close()


def test_wrong_sizes_are_refused_before_launch(hal):
    """wrong program_rows / muldiv_rows and too many segments: nothing is written (every buffer keeps its fill pattern)"""
    lib = _lib.load()
    elf = MP.m_program(1)
    key = X.setup_rv32_elf(hal, elf)
    st = X.Stepper(elf, INPUT, 13)
    try:
        more = C.c_int(0)
        _lib.check(None, lib.rk_exec_next_segment(st._h, C.byref(more)))
        md = C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32im_sizes(st._h, 0, C.byref(md)))
        rows = 1 << key.program_log_height
        assert md.value == 1024 and rows == 1024
        logs = [13, key.program_log_height, 5, 18, 16, 12, 10]
        bufs = [hal.alloc_elem(a.width << lg) for a, lg in zip(key.airs, logs)]
        try:
            for b in bufs:
                b.copy_from(np.full(b.words, 7, dtype=np.uint32))
            ptrs = [C.c_void_p(b.ptr) for b in bufs]
            u = lambda a: a.ctypes.data_as(_lib.u32p)
            seg = (u(key.seg_vaddr), u(key.seg_words), key.seg_vaddr.size, C.c_void_p(key.d_words.ptr))
            call = lambda seg, prog_rows, md_rows: lib.rk_exec_rv32elf_shard_device(hal._ctx, st._h, 0, *seg, ptrs[0], ptrs[1], prog_rows,
                                                                                    *ptrs[2:], md_rows)
            assert call(seg, rows // 2, md.value) == _lib.RK_ERR_CAPACITY
            assert call(seg, rows * 2, md.value) == _lib.RK_ERR_CAPACITY
            assert call(seg, rows, 512) == _lib.RK_ERR_CAPACITY
            assert call(seg, rows, 1536) == _lib.RK_ERR_INVALID
            many_v, many_w = np.arange(17, dtype=np.uint32) * 64 + 0x1000, np.ones(17, dtype=np.uint32)
            assert call((u(many_v), u(many_w), 17, C.c_void_p(key.d_words.ptr)), 32, md.value) == _lib.RK_ERR_INVALID
            # the preprocessed matrices: wrong program_rows, too many segments, seg_words that do not sum to n_words
            words = np.concatenate([w for _v, w in key.image]).astype(np.uint32)
            prep = lambda v, w, n, n_words, prog_rows: lib.rk_rv32elf_prep_device(hal._ctx, u(v), u(w), n, u(words), n_words, ptrs[0], prog_rows,
                                                                                 ptrs[3], ptrs[4], ptrs[5])
            assert prep(key.seg_vaddr, key.seg_words, 2, words.size, rows // 2) == _lib.RK_ERR_CAPACITY
            assert prep(many_v, many_w, 17, 17, 32) == _lib.RK_ERR_INVALID
            assert prep(key.seg_vaddr, key.seg_words, 2, words.size - 1, rows) == _lib.RK_ERR_INVALID
            hal.sync()
            assert all((b.to_host() == 7).all() for b in bufs)
            _lib.check(hal._ctx, call(seg, rows, md.value))       # the right sizes work
            hal.sync()
            assert not (bufs[1].to_host() == 7).all()
        finally:
            for b in bufs:
                b.free()
    finally:
        st.close()
        key.close()


def test_self_modifying_guest_is_refused(hal):
    elf = EP.selfmod_program()
    key = X.setup_rv32_elf(hal, elf)
    try:
        with pytest.raises(_lib.RkError) as e:
            X.execute_rv32_device(hal, elf, INPUT, 13, chips="rv32im-elf", key=key)
        assert e.value.status == _lib.RK_ERR_INVALID
        # rv32im writes its tables without complaint: the gap
        _ex, _shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, 13, chips="rv32im")
        free(bufs)
    finally:
        key.close()


@pytest.mark.parametrize("preset", [0, 1])
def test_execute_and_prove_and_pipeline(preset):
    """the public entry points under both parameter sets: every shard verifies against the one root, the chain check
    passes (inside), pipeline proofs = prove_shards' words = the words of proofs made from the numpy tables
    (Table(prep=) + p3.setup on a single context)"""
    blob = H.make_params(preset, **FAST)
    elf = MP.m_program(25)
    ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=13, params=blob, batch=2, chips="rv32im-elf")
    assert len(proofs) == len(ex.segments) >= 3 and ex.prep_root is not None and ex.program_log_height == 10
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc, prep_root=ex.prep_root,
                                   program_log_height=ex.program_log_height)
    for (tables, init), pf in zip(shards, proofs):
        assert X.verify_rv32_shard(tables, pf, init, blob, prep_root=ex.prep_root, program_log_height=ex.program_log_height) == 0
        assert X.verify_rv32_shard(tables, pf, init, blob, prep_root=ex.prep_root, program_log_height=11) != 0   # the height is the verifier's
    ex2, pproofs, kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=13, params=blob, chips="rv32im-elf", keep_tables=True)
    assert np.array_equal(ex2.prep_root, ex.prep_root) and len(pproofs) == len(proofs)
    for a, b in zip(pproofs, proofs):
        assert np.array_equal(a, b)
    # the numpy route
    image = rv32elf.program_image(elf)
    ref = X.p3_rv32elf_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True), image, ext_w=int(blob.ext_w))
    h = H.HipHal(0)
    try:
        _lib.check(h._ctx, h._lib.rk_set_params(h._ctx, C.byref(blob)))
        key = p3.setup(h, ref[0][0])
        try:
            assert np.array_equal(key.root, ex.prep_root)
            for (tables, init), pf, (kt, kinit) in zip(ref, proofs, kept):
                assert np.array_equal(p3.prove(h, tables, init, key=key), pf)
                for t, r in zip(kt, tables):
                    assert np.array_equal(t.trace, r.trace) and (r.prep is None or np.array_equal(t.prep, r.prep))
        finally:
            key.close()
    finally:
        h.close()


def test_the_root_names_the_program(hal):
    """two ELFs that differ in one immediate of an instruction that executes: under rv32im each run's proofs verify with
    nothing naming the program; under rv32im-elf run A verifies against root A and is refused against root B"""
    blob = H.make_params(1, **FAST)
    elf_a, elf_b = EP.imm_program(5), EP.imm_program(6)
    for elf in (elf_a, elf_b):
        ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=13, params=blob, chips="rv32im")
        assert X.verify_rv32_execution(shards, proofs, blob)          # the statement has no place for the program
    exa, sha, pfa = X.execute_and_prove_p3(elf_a, INPUT, shard_po2=13, params=blob, chips="rv32im-elf")
    exb, shb, pfb = X.execute_and_prove_p3(elf_b, INPUT, shard_po2=13, params=blob, chips="rv32im-elf")
    assert not np.array_equal(exa.prep_root, exb.prep_root) and exa.program_log_height == exb.program_log_height
    vk = lambda ex: dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height)
    (ta, ia), (tb, ib) = sha[0], shb[0]
    assert X.verify_rv32_shard(ta, pfa[0], ia, blob, **vk(exa)) == 0 and X.verify_rv32_shard(tb, pfb[0], ib, blob, **vk(exb)) == 0
    assert X.verify_rv32_shard(ta, pfa[0], ia, blob, **vk(exb)) != 0
    assert X.verify_rv32_shard(tb, pfb[0], ib, blob, **vk(exa)) != 0
    with pytest.raises(ValueError):
        X.verify_rv32_execution(sha, pfa, blob, **vk(exb))
    # setup twice on one ELF: the same root
    k1 = X.setup_rv32_elf(hal, elf_a, blob)
    k2 = X.setup_rv32_elf(hal, elf_a, blob)
    try:
        assert np.array_equal(k1.root, k2.root) and np.array_equal(k1.root, exa.prep_root)
        assert k1.bytes > (42 << 11) * 4
    finally:
        k1.close()
        k2.close()


def test_unused_image_rows_keep_multiplicity_zero():
    blob = H.make_params(1, **FAST)
    elf = EP.unused_rows_program()
    ex, proofs, kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=13, params=blob, chips="rv32im-elf", keep_tables=True)
    (tables, init), = kept
    mult = p3.from_mont(tables[1].trace)[:, 0]
    assert mult[:2].tolist() == [1, 1] and mult[2:5].tolist() == [0, 0, 0] and mult[5] == 1 and mult.sum() == ex.segments[0].cycles
    assert X.verify_rv32_shard(tables, proofs[0], init, blob, prep_root=ex.prep_root, program_log_height=ex.program_log_height) == 0
