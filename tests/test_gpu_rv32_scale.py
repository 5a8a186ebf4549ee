"""The rv32 witness kernels at the scale of a production shard: every table rk_exec_rv32mem_shard_device and
rk_exec_rv32_shard_device write against the numpy witness, word for word, on shards whose access lists fill hundreds of
128-position blocks -- one past what mscan_kernel's 1 024 lanes take one block each of --, whose sorted order is unrelated
to their list order, whose memop table is as tall as the cpu table or twice as tall, with 16 000 accesses at one cycle,
with thousands of accesses at sixteen words; and on shards whose register reads find their predecessor several of
scan_kernel's chunks back.  tests/test_rv32_scale.py holds that the guests are these shapes and holds the numpy witness
at two of them; tests/test_gpu_rv32_mem_chips.py and tests/test_gpu_rv32_chips.py run the small ones.

The device's own cross-checks (a row count that is not the host's, an access that is not its instruction's) raise
RkError from execute_rv32_device: a failure here, not something to catch."""
import ctypes as C

import numpy as np
import pytest

import rv32_mem_programs as GP
import rv32_scale_programs as SP
from raiko_amd import _lib, rv32elf, rv32mem
from raiko_amd import executor as X
from raiko_amd import hal as H
from test_gpu_rv32_mem_chips import _witness_key

pytestmark = pytest.mark.gpu

FAST = dict(queries=8, pow_bits=6)
GAP_INPUT = [11, 22, 33, 44]


@pytest.fixture(scope="module")
def hal():
    h = H.HipHal(0)
    h.set_params(1, **FAST)
    yield h
    h.close()


@pytest.fixture(scope="module")
def airs(hal):
    return rv32mem.airs(int(hal.get_params().ext_w))


def _equal(shards, bufs, ref):
    """all tables and public values of every shard, device against numpy; the first differing word is named"""
    assert len(ref) == len(shards) == len(bufs)
    for k, ((rt, rinit), d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
        assert np.array_equal(init, rinit) and len(d) == len(rt) == len(tables)
        for i, (r, (b, lg), t) in enumerate(zip(rt, d, tables)):
            assert (1 << lg, t.air.width) == r.trace.shape, (k, i, lg)
            g = b.to_host().reshape(r.trace.shape)
            bad = np.nonzero(g != r.trace)
            assert bad[0].size == 0, "shard %d table %d: first difference at row %d col %d (%d of %d words differ)" % (
                k, i, bad[0][0], bad[1][0], bad[0].size, g.size)
            assert np.array_equal(t.public_values, r.public_values), (k, i)


def _free(bufs):
    for d in bufs:
        for b, _ in d:
            b.free()


def _mem_case(hal, airs, elf, inp, po2):
    """elf through rk_exec_rv32mem_shard_device and through the numpy witness -> the numpy shards' cpu-table heights and
    (accesses, memop rows, memory rows) per shard, after every table compared equal"""
    image = rv32elf.program_image(elf)
    key = _witness_key(hal, elf, airs)
    try:
        _ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, inp, po2, chips="rv32im-mem", key=key)
        try:
            hal.sync()
            ref_ex = X.execute(elf, inp, segment_limit_po2=po2, record_trace=True)
            ref = X.p3_rv32mem_shards(ref_ex, image, airs=airs)
            _equal(shards, bufs, ref)
            return [(t[0].trace.shape[0], len(m), t[7].trace.shape[0], t[8].trace.shape[0]) for (t, _i), m in zip(ref, ref_ex.mem)]
        finally:
            _free(bufs)
    finally:
        key.d_words.free()


def test_memop_as_tall_as_the_cpu_table(hal, airs):
    """63 547 accesses at 16 words: runs of thousands (the far end of mem_link_kernel's binary search, hist_add under
    equal values), a memory table of one tile beside 497 blocks of sorted positions; and a second, short shard"""
    got = _mem_case(hal, airs, GP.loadstore_loop(1100), [], 16)
    assert got == [(65536, 63547, 65536, 16), (8192, 6853, 8192, 16)]


def test_scattered_accesses(hal, airs):
    """21 500 accesses at 12 284 words in no order: the sort's result and its stability, the heads compacted over 168
    blocks"""
    assert _mem_case(hal, airs, SP.scatter_program(4300), [], 16) == [(65536, 21500, 32768, 16384)]


def test_16000_accesses_at_one_cycle(hal, airs):
    """an ecall READ of 16 000 words: both tables twice the cpu table's height, N_ECW of one row counted 16 000 times"""
    assert _mem_case(hal, airs, GP.big_read_program(16000), list(range(1, 16385)), 13) == [(8192, 16000, 16384, 16384)]


def test_accesses_at_the_cap_and_one_past_it(hal, airs):
    """16 384 accesses in a 2^13-row shard: exactly the cap, no padding row in either table.  One more is refused before
    any launch, whatever heights the caller offers -- by the very call, on the same buffers, that writes the guest at
    the cap (so the refusal is of the access count, not of an argument this test got wrong)"""
    assert _mem_case(hal, airs, GP.big_read_program(16384), list(range(1, 16385)), 13) == [(8192, 16384, 16384, 16384)]
    words = 16385
    ex = X.execute(GP.big_read_program(words), list(range(1, words + 1)), segment_limit_po2=13, record_trace=True)
    assert len(ex.segments) == 1 and ex.segments[0].po2 == 13 and len(ex.mem[0]) == words
    with pytest.raises(ValueError, match="more accesses than twice"):
        X.p3_rv32mem_shards(ex, rv32elf.program_image(GP.big_read_program(words)), airs=airs)
    lib = _lib.load()
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    bufs = None
    try:
        for words in (16384, 16385):
            elf, inp = GP.big_read_program(words), list(range(1, words + 1))
            key = _witness_key(hal, elf, airs)
            st = X.Stepper(elf, inp, 13)
            try:
                more = C.c_int(0)
                _lib.check(None, lib.rk_exec_next_segment(st._h, C.byref(more)))
                md, mo, bd = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
                _lib.check(None, lib.rk_exec_rv32im_sizes(st._h, 0, C.byref(md)))
                logs = [13, key.program_log_height, 5, 18, 16, 12, md.value.bit_length() - 1, 15, 15]   # memop / memory: room for every size tried
                if bufs is None:
                    shape = logs
                    bufs = [hal.alloc_elem(a.width << lg) for a, lg in zip(airs, logs)]
                assert logs == shape                                       # both guests take the same buffers
                for b in bufs:
                    b.copy_from(np.full(b.words, 7, dtype=np.uint32))
                ptrs = [C.c_void_p(b.ptr) for b in bufs]
                call = lambda mo_rows, bd_rows: lib.rk_exec_rv32mem_shard_device(
                    hal._ctx, st._h, 0, u(key.seg_vaddr), u(key.seg_words), key.seg_vaddr.size, C.c_void_p(key.d_words.ptr), ptrs[0], ptrs[1],
                    1 << key.program_log_height, *ptrs[2:7], md.value, ptrs[7], mo_rows, ptrs[8], bd_rows)
                if words == 16384:
                    _lib.check(None, lib.rk_exec_rv32mem_sizes(st._h, 0, C.byref(mo), C.byref(bd)))
                    assert (mo.value, bd.value) == (1 << 14, 1 << 14)
                    _lib.check(hal._ctx, call(1 << 14, 1 << 14))
                    hal.sync()
                    assert not any((b.to_host()[: a.width << lg] == 7).all() for a, b, lg in zip(airs, bufs, logs[:7] + [14, 14]))
                else:
                    assert lib.rk_exec_rv32mem_sizes(st._h, 0, C.byref(mo), C.byref(bd)) == _lib.RK_ERR_CAPACITY
                    # 2^14 rows do not hold the accesses, 2^15 are more than twice the cpu table
                    for mo_rows, bd_rows in ((1 << 14, 1 << 14), (1 << 15, 1 << 15), (1 << 15, 1 << 14), (1 << 14, 1 << 15)):
                        assert call(mo_rows, bd_rows) == _lib.RK_ERR_INVALID, (mo_rows, bd_rows)
                    hal.sync()
                    assert all((b.to_host() == 7).all() for b in bufs)
            finally:
                st.close()
                key.d_words.free()
    finally:
        for b in bufs or []:
            b.free()


def test_1024_blocks_of_accesses(hal, airs):
    """131 072 accesses = 1 024 blocks of 128: mscan_kernel's lanes take one block each; memop exactly full"""
    got = _mem_case(hal, airs, SP.scatter_program(8700, pre_read=87572), list(range(1, 140001)), 17)
    assert got == [(131072, 131072, 131072, 131072)]


def test_1025_blocks_of_accesses(hal, airs):
    """131 073 accesses = 1 025 blocks: one lane of mscan_kernel sums two blocks; memop twice the cpu table's height"""
    got = _mem_case(hal, airs, SP.scatter_program(8700, pre_read=87573), list(range(1, 140001)), 17)
    assert got == [(131072, 131073, 262144, 131072)]


@pytest.mark.parametrize("po2,tail_spin", [(13, 3000), (16, 34000)])
def test_far_register_predecessors_rv32i(hal, po2, tail_spin):
    """gap_program under rv32i: reads whose predecessor lies in the row, the wave, the block, the block before and
    several chunks back (tests/test_rv32_scale.py counts them)"""
    elf = SP.gap_program(SP.GAPS, tail_spin)
    i_airs = X.p3_rv32_airs(int(hal.get_params().ext_w))
    _ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, GAP_INPUT, po2, airs=i_airs, chips="rv32i")
    try:
        hal.sync()
        ref_ex = X.execute(elf, GAP_INPUT, segment_limit_po2=po2, record_trace=True)
        assert len(ref_ex.segments) == 2 and ref_ex.segments[0].cycles == 1 << po2
        _equal(shards, bufs, X.p3_rv32_shards(ref_ex, airs=i_airs))
    finally:
        _free(bufs)


def test_far_register_predecessors_rv32im_mem(hal, airs):
    """the same guest through rows_kernel with the widest row"""
    got = _mem_case(hal, airs, SP.gap_program(SP.GAPS, 3000), GAP_INPUT, 13)
    assert got == [(8192, 0, 2, 2), (8192, 0, 2, 2)]
