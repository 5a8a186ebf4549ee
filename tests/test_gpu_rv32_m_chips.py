"""The rv32im chip set on the GPU: rk_exec_rv32im_shard_device's tables against the numpy reference (p3_rv32im_shards),
word for word; proofs against the CPU oracle; the public entry points verified and chained; a muldiv buffer too small
for the segment refused before any launch; and the forgery rv32i-cf cannot see (a wrong MUL result) accepted under
rv32i-cf, refused under rv32im."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as o
import rv32_cf_programs as CP
import rv32_m_programs as MP
from raiko_amd import _lib, p3, rv32im
from raiko_amd import executor as X
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

INPUT = [11, 22, 33, 44]
FAST = dict(queries=8, pow_bits=6)


@pytest.fixture(scope="module")
def hal():
    h = H.HipHal(0)
    yield h
    h.close()
    o.oracle_set_params()


def free(bufs):
    for d in bufs:
        for b, _ in d:
            b.free()


@pytest.mark.parametrize("name,po2", [("m1", 13), ("m25", 13), ("mixed", 16), ("none", 13), ("mixed", 13)])
def test_device_tables_equal_numpy(hal, name, po2):
    """one shard, several shards with a partial last one, a 2^16 shard, a shard with no M instruction, a mixed loop:
    every device-written table = the numpy one"""
    elf = {"m1": MP.m_program(1), "m25": MP.m_program(25), "mixed": MP.mixed_program(400), "none": CP.cf_program(1)}[name]
    airs = X.p3_rv32im_airs()
    ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, po2, airs=airs, chips="rv32im")
    try:
        hal.sync()
        ref_ex = X.execute(elf, INPUT, segment_limit_po2=po2, record_trace=True)
        ref = X.p3_rv32im_shards(ref_ex, airs=airs)
        assert len(ref) == len(shards) == len(bufs)
        if name == "m25":
            assert len(ref) > 1 and ref_ex.segments[-1].cycles < 1 << ref_ex.segments[-1].po2
        for k, ((rt, rinit), d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
            assert np.array_equal(init, rinit)
            assert len(d) == 7
            for i, (r, (b, lg), t) in enumerate(zip(rt, d, tables)):
                g = b.to_host().reshape(1 << lg, t.air.width)
                assert g.shape == r.trace.shape, (k, i)
                bad = np.nonzero(g != r.trace)
                assert bad[0].size == 0, "shard %d table %d: first difference at row %d col %d" % (k, i, bad[0][0], bad[1][0])
                assert np.array_equal(t.public_values, r.public_values)
    finally:
        free(bufs)


def test_rv32cf_device_tables_unchanged(hal):
    """rk_exec_rv32cf_shard_device beside the new entry point: its tables are still the numpy rv32i-cf ones"""
    elf = MP.m_program(25)
    ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, 13, chips="rv32i-cf")
    ref = X.p3_rv32cf_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True))
    try:
        hal.sync()
        for (rt, _), d, (tables, _) in zip(ref, bufs, shards):
            for r, (b, lg), t in zip(rt, d, tables):
                assert np.array_equal(b.to_host().reshape(1 << lg, t.air.width), r.trace)
    finally:
        free(bufs)


def test_small_muldiv_buffer_refused_before_launch(hal):
    """a muldiv row count below what the segment needs: RK_ERR_CAPACITY, and no table is written"""
    lib = _lib.load()
    st = X.Stepper(MP.m_program(1), INPUT, 13)
    try:
        more = C.c_int(0)
        _lib.check(None, lib.rk_exec_next_segment(st._h, C.byref(more)))
        rows, md = C.c_size_t(0), C.c_size_t(0)
        _lib.check(None, lib.rk_exec_rv32_sizes(st._h, 0, C.byref(rows)))
        _lib.check(None, lib.rk_exec_rv32im_sizes(st._h, 0, C.byref(md)))
        assert md.value == 1024
        airs = X.p3_rv32im_airs()
        logs = [13, rows.value.bit_length() - 1, 5, 18, 16, 12, 10]
        bufs = [hal.alloc_elem(a.width << lg) for a, lg in zip(airs, logs)]
        try:
            for b in bufs:
                b.copy_from(np.full(b.words, 7, dtype=np.uint32))
            ptrs = [C.c_void_p(b.ptr) for b in bufs]
            rc = lib.rk_exec_rv32im_shard_device(hal._ctx, st._h, 0, ptrs[0], ptrs[1], rows.value, *ptrs[2:], 512)
            assert rc == _lib.RK_ERR_CAPACITY
            rc = lib.rk_exec_rv32im_shard_device(hal._ctx, st._h, 0, ptrs[0], ptrs[1], rows.value, *ptrs[2:], 1536)
            assert rc == _lib.RK_ERR_INVALID
            hal.sync()
            assert all((b.to_host() == 7).all() for b in bufs)
            # the right size works
            _lib.check(hal._ctx, lib.rk_exec_rv32im_shard_device(hal._ctx, st._h, 0, ptrs[0], ptrs[1], rows.value, *ptrs[2:],
                                                                  md.value))
            hal.sync()
        finally:
            for b in bufs:
                b.free()
    finally:
        st.close()


def test_proof_words_equal_oracle_and_run_verifies(hal):
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    elf = MP.m_program(25)
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    shards = X.p3_rv32im_shards(ex)
    assert len(shards) >= 3
    tables, init = shards[0]
    got = p3.prove(hal, tables, init)
    assert np.array_equal(got, o.oracle_p3_prove(tables, init))
    proofs = p3.prove_shards(shards, blob, batch=2, verify=True)
    assert np.array_equal(proofs[0], got)
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc)


def test_forgery_rv32cf_accepts_and_rv32im_refuses(hal):
    """THE GAP: a one-row MUL with a wrong result proves and verifies under rv32i-cf (reason 0) and is refused under
    rv32im (reason 3, the muldiv constraint); both proofs equal the oracle's"""
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    init = np.zeros(16, dtype=np.uint32)
    for chips, airs, want in (("rv32i-cf", X.p3_rv32cf_airs(), 0), ("rv32im", X.p3_rv32im_airs(), 3)):
        canon, pub_cpu, pub_reg = MP.one_row(chips, **MP.MUL_WRONG)
        tables = [p3.Table.from_canonical(a, t, pv) for a, t, pv in zip(airs, canon, [pub_cpu, (), pub_reg, (), (), (), ()])]
        pf = p3.prove(hal, tables, init)
        assert np.array_equal(pf, o.oracle_p3_prove(tables, init)), chips
        assert X.verify_rv32_shard(tables, pf, init, blob) == want, chips


@pytest.mark.parametrize("preset", [0, 1])
def test_execute_and_prove_rv32im(hal, preset):
    """the public entry point, device tables, under both parameter sets: proofs = the host-table route's"""
    blob = H.make_params(preset, **FAST)
    elf = MP.m_program(25)
    ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=13, params=blob, batch=2, chips="rv32im")
    assert len(proofs) == len(ex.segments) >= 3
    ref = X.p3_rv32im_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True), ext_w=int(blob.ext_w))
    ref_proofs = p3.prove_shards(ref, blob, batch=2, verify=True)
    for a, b in zip(proofs, ref_proofs):
        assert np.array_equal(a, b)


def test_pipeline_rv32im_equals_host_route(hal):
    blob = H.make_params(1, **FAST)
    elf = MP.m_program(25)
    ex, proofs, kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=13, params=blob, chips="rv32im",
                                                        keep_tables=True)
    ref = X.p3_rv32im_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True), ext_w=int(blob.ext_w))
    ref_proofs = p3.prove_shards(ref, blob, batch=2, verify=True)
    assert len(proofs) == len(ref_proofs) == len(ex.segments) >= 3
    for a, b in zip(proofs, ref_proofs):
        assert np.array_equal(a, b)
    for (tables, init), (rt, rinit) in zip(kept, ref):
        assert np.array_equal(init, rinit)
        for t, r in zip(tables, rt):
            assert np.array_equal(t.trace, r.trace)
    assert X.verify_rv32_execution(kept, proofs, blob, entry_pc=ex.segments[0].start_pc)
    assert rv32im.BUS_MULDIV == 8
