"""The rv32im-mem chip set on the GPU: rk_rv32mem_prep_device's program matrix and rk_exec_rv32mem_shard_device's nine
traces against raiko_amd/rv32mem.py's numpy, word for word (the count columns included), at access counts around the
kernels' 128-row tile, with one long chain and with every access at a word of its own; wrong sizes refused before any
launch; one ELF through setup, the keyed shard pool and the verifier; and proofs refused against the key of an ELF that
differs in one store immediate.

The numpy tables are held to the AIRs and the buses in tests/test_rv32_mem_chips.py; the keyed prover to the exact
reference in tests/test_gpu_p3_shards_key.py."""
import ctypes as C
import types

import numpy as np
import pytest

import rv32_mem_programs as GP
from raiko_amd import _lib, p3, rv32elf, rv32mem
from raiko_amd import executor as X
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

INPUT = [0x11223344, 0x80FF7F01, 0xDEADBEEF, 0x00000044]
FAST = dict(queries=8, pow_bits=6)
PROGRAMS = dict(GP.GUESTS, two=GP.two_shard_program, forge=GP.forge_program)
PROGRAMS.update({"count%d" % k: (lambda k=k: GP.count_program(k)) for k in (0, 1, 2, 128, 129)})   # one LDS tile and one past it
PROGRAMS.update(one_word=lambda: GP.count_program(300), distinct=lambda: GP.count_program(300, distinct=True))


@pytest.fixture(scope="module")
def hal():
    h = H.HipHal(0)
    h.set_params(1, **FAST)
    yield h
    h.close()


@pytest.fixture(scope="module")
def airs(hal):
    return rv32mem.airs(int(hal.get_params().ext_w))


def _witness_key(hal, elf, airs):
    """what rk_exec_rv32mem_shard_device needs of a key -- the image's segments and its words in device memory --
    without the commitment (setup_rv32_elf's cost, which test_execute_and_prove pays once)"""
    vaddr, count, words = X.program_image_c(elf)
    rows = 2
    while rows < words.size:
        rows <<= 1
    d_words = hal.copy_from_elem(words)
    hal.sync()
    stub = types.SimpleNamespace(root=None, bytes=0, close=lambda: None)
    return X.Rv32Key(rv32elf.program_image(elf), vaddr, count, stub, d_words, rows.bit_length() - 1, airs, "rv32im-mem")


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_device_tables_equal_numpy(hal, airs, name):
    elf = PROGRAMS[name]()
    image = rv32elf.program_image(elf)
    key = _witness_key(hal, elf, airs)
    try:
        ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, 13, chips="rv32im-mem", key=key)
        try:
            hal.sync()
            ref_ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
            ref = X.p3_rv32mem_shards(ref_ex, image, airs=airs)
            assert len(ref) == len(shards) == len(bufs) == (2 if name == "two" else 1)
            for k, ((rt, rinit), d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
                assert np.array_equal(init, rinit) and len(d) == 9
                for i, (r, (b, lg), t) in enumerate(zip(rt, d, tables)):
                    g = b.to_host().reshape(1 << lg, t.air.width)
                    assert g.shape == r.trace.shape, (k, i)
                    bad = np.nonzero(g != r.trace)
                    assert bad[0].size == 0, "shard %d table %d: first difference at row %d col %d" % (k, i, bad[0][0], bad[1][0])
                    assert np.array_equal(t.public_values, r.public_values)
            memop, memory = (p3.from_mont(ref[0][0][i].trace) for i in (7, 8))
            n_acc, n_words = int(memop[:, rv32mem.G_MULT].sum()), int(memory[:, rv32mem.B_REAL].sum())
            if name.startswith("count"):
                assert n_acc == int(name[5:]) and n_words == min(n_acc, 1)
                assert memop.shape[0] == {0: 2, 1: 2, 2: 2, 128: 128, 129: 256}[n_acc]
            if name == "one_word":      # one boundary row and one long chain
                assert (n_acc, n_words) == (300, 1) and memory.shape[0] == 2 and (memop[1:300, rv32mem.G_PTS] == memop[:299, rv32mem.G_TS]).all()
            if name == "distinct":      # the memory table as tall as memop
                assert (n_acc, n_words) == (300, 300) and memory.shape[0] == memop.shape[0] == 512
        finally:
            for d in bufs:
                for b, _ in d:
                    b.free()
    finally:
        key.d_words.free()


def test_program_matrix_equals_numpy(hal):
    lib = _lib.load()
    for elf in (GP.ops_program(), GP.count_program(300, distinct=True)):
        want = p3.to_mont(rv32mem.prep_tables(rv32elf.program_image(elf))[0])
        vaddr, count, words = X.program_image_c(elf)
        bufs = [hal.alloc_elem(s) for s in (want.size, 4 << 18, 1 << 16, 4 << 12)]
        try:
            ptr = lambda a: a.ctypes.data_as(_lib.u32p)
            _lib.check(hal._ctx, lib.rk_rv32mem_prep_device(hal._ctx, ptr(vaddr), ptr(count), vaddr.size, ptr(words), words.size,
                                                            C.c_void_p(bufs[0].ptr), want.shape[0], *[C.c_void_p(b.ptr) for b in bufs[1:]]))
            hal.sync()
            assert np.array_equal(bufs[0].to_host().reshape(want.shape), want)
            assert np.array_equal(bufs[2].to_host(), p3.to_mont(np.arange(1 << 16)))
        finally:
            for b in bufs:
                b.free()


def test_wrong_sizes_are_refused_before_launch(hal, airs):
    """memop / memory buffers smaller than rk_exec_rv32mem_sizes gives, no power of two, or taller than twice the cpu
    table: RK_ERR_INVALID and nothing is written (every buffer keeps its fill pattern)"""
    lib = _lib.load()
    elf = GP.count_program(129, distinct=True)
    key = _witness_key(hal, elf, airs)
    st = X.Stepper(elf, INPUT, 13)
    try:
        more = C.c_int(0)
        _lib.check(None, lib.rk_exec_next_segment(st._h, C.byref(more)))
        md, mo, bd = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32im_sizes(st._h, 0, C.byref(md)))
        _lib.check(None, lib.rk_exec_rv32mem_sizes(st._h, 0, C.byref(mo), C.byref(bd)))
        assert (md.value, mo.value, bd.value) == (2, 256, 256)
        logs = [13, key.program_log_height, 5, 18, 16, 12, 1, 15, 15]          # memop / memory: room for every size tried
        bufs = [hal.alloc_elem(a.width << lg) for a, lg in zip(airs, logs)]
        try:
            for b in bufs:
                b.copy_from(np.full(b.words, 7, dtype=np.uint32))
            ptrs = [C.c_void_p(b.ptr) for b in bufs]
            u = lambda a: a.ctypes.data_as(_lib.u32p)
            call = lambda mo_rows, bd_rows: lib.rk_exec_rv32mem_shard_device(
                hal._ctx, st._h, 0, u(key.seg_vaddr), u(key.seg_words), key.seg_vaddr.size, C.c_void_p(key.d_words.ptr), ptrs[0], ptrs[1],
                1 << key.program_log_height, *ptrs[2:7], md.value, ptrs[7], mo_rows, ptrs[8], bd_rows)
            for mo_rows, bd_rows in ((128, 256), (256, 128), (384, 256), (256, 384), (1 << 15, 256), (256, 1 << 15), (0, 256)):
                assert call(mo_rows, bd_rows) == _lib.RK_ERR_INVALID, (mo_rows, bd_rows)
            hal.sync()
            assert all((b.to_host() == 7).all() for b in bufs)
            _lib.check(hal._ctx, call(512, 1 << 14))                           # taller powers of two up to 2^(po2 + 1) work
            hal.sync()
            memop = p3.from_mont(bufs[7].to_host()[: 512 * 64]).reshape(512, 64)
            memory = p3.from_mont(bufs[8].to_host()[: (1 << 14) * 13]).reshape(1 << 14, 13)
            assert memop[:, rv32mem.G_MULT].sum() == 129 and (memop[:, rv32mem.G_ONE] == 1).all()
            assert memory[:, rv32mem.B_REAL].sum() == 129 and not memory[129:].any()
        finally:
            for b in bufs:
                b.free()
    finally:
        st.close()
        key.d_words.free()


def test_execute_and_prove_and_the_key_names_the_program():
    """the two-shard guest through setup -> rk_p3_prove_shards_key -> verify_rv32_execution (the registers and pcs
    chain; the shards' memories do not: INIT is free), and proofs of one ELF refused against the key of an ELF that
    differs in one store immediate"""
    blob = H.make_params(1, **FAST)
    ex, shards, proofs = X.execute_and_prove_p3(GP.two_shard_program(), INPUT, shard_po2=13, params=blob, batch=2, chips="rv32im-mem")
    assert len(proofs) == len(ex.segments) == 2 and ex.prep_root is not None
    vk = lambda e: dict(prep_root=e.prep_root, program_log_height=e.program_log_height)
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc, **vk(ex))
    tables, init = shards[0]
    assert len(tables) == 9 and [int(proofs[0][1 + i]) for i in (7, 8)] == [1, 1]      # two accesses, two words
    # the pipeline (executor, witness and prover overlapped) writes the same proofs under the same root
    ex2, pproofs, _kept = X.execute_and_prove_p3_pipelined(GP.two_shard_program(), INPUT, shard_po2=13, params=blob, chips="rv32im-mem")
    assert np.array_equal(ex2.prep_root, ex.prep_root) and len(pproofs) == 2
    assert all(np.array_equal(a, b) for a, b in zip(pproofs, proofs))
    exa, sha, pfa = X.execute_and_prove_p3(GP.store_imm_program(8), INPUT, shard_po2=13, params=blob, chips="rv32im-mem")
    exb, shb, pfb = X.execute_and_prove_p3(GP.store_imm_program(12), INPUT, shard_po2=13, params=blob, chips="rv32im-mem")
    assert not np.array_equal(exa.prep_root, exb.prep_root) and exa.program_log_height == exb.program_log_height
    (ta, ia), (tb, ib) = sha[0], shb[0]
    assert X.verify_rv32_shard(ta, pfa[0], ia, blob, **vk(exa)) == 0 and X.verify_rv32_shard(tb, pfb[0], ib, blob, **vk(exb)) == 0
    assert X.verify_rv32_shard(ta, pfa[0], ia, blob, **vk(exb)) != 0
    assert X.verify_rv32_shard(tb, pfb[0], ib, blob, **vk(exa)) != 0
    with pytest.raises(ValueError):
        X.verify_rv32_execution(sha, pfa, blob, **vk(exb))
    # the heights of memop and memory are the proof's, bounded by the verifier: a claim past 2^(po2 + 1) is refused
    forged = pfa[0].copy()
    forged[1 + 7] = 15
    assert X.verify_rv32_shard(ta, forged, ia, blob, **vk(exa)) == 2
