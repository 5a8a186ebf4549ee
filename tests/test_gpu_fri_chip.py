"""rk_fri_chip_rows_device on the GPU (raiko_amd/fri_chip.py): the rows of the four FRI commit-phase tables equal the
numpy witness word for word; the tables stay in HBM and go to rk_p3_prove as on_device tables, whose proof is the
oracle's over the witness; verify_fri_statement accepts it; an undersized buffer is refused before anything is written."""
import ctypes as C

import numpy as np
import pytest

import fri_param_sets as PS
import oracle_lib as o
from p3_cases import P3_CASES, init_of, tables_of
from raiko_amd import _lib, hal, p3
from raiko_amd import fri_chip as F
from raiko_amd.hal import _ptr

pytestmark = pytest.mark.gpu


def shard(h, case, pset=None, **more):
    """the shard proof of `case` on the GPU, under the case's own parameters or under a set of tests/fri_param_sets.py"""
    if pset is None:
        preset, over, _, _ = P3_CASES[case]
        tables, init = tables_of(case), init_of(case)
    else:
        preset, over = PS.shard_params(pset, case)
        tables, init = PS.shard_tables(pset, case)
    over = dict(over, **more)
    blob = h.set_params(preset, **over)
    o.oracle_set_params(preset, **over)
    pf = p3.prove(h, tables, init)
    return blob, tables, init, pf


@pytest.mark.parametrize("case", ["sp1_mixed_fib8_cubic4", "sp1_blow2_wide_k9"])
def test_gpu_rows_equal_the_witness(case):
    h = hal.HipHal(0)
    try:
        blob, tables, init, pf = shard(h, case)
        assert np.array_equal(pf, o.oracle_p3_prove(tables, init))
        st = F.statement(tables, pf, init, blob)
        want = [p3.to_mont(r) for r in F.witness(st)]
        dev = F.device_tables(h, st)
        assert [lh for _, lh in dev] == list(F.heights(st.shape))
        for (buf, lh), w in zip(dev, want):
            got = buf.to_host().reshape(w.shape)
            assert np.array_equal(got, w), np.argwhere(got != w)[:8]
    finally:
        o.oracle_set_params()
        h.close()


@pytest.mark.parametrize("pset,case", PS.ROW_IDS, ids=[PS.row_id(*x) for x in PS.ROW_IDS])
def test_gpu_rows_under_parameter_sets(pset, case):
    """fri_path_kernel<0> and <1>, the chip under other tables, the fold chain in another field, blow-ups 8 and 16"""
    h = hal.HipHal(0)
    try:
        blob, tables, init, pf = shard(h, case, pset)
        ctx = h.get_params()
        assert (ctx.p2_m4, ctx.ext_w, ctx.blowup_log2) == (blob.p2_m4, blob.ext_w, blob.blowup_log2)
        assert np.array_equal(pf, o.oracle_p3_prove(tables, init))
        st = F.statement(tables, pf, init, blob)
        want = [p3.to_mont(r) for r in F.witness(st)]
        dev = F.device_tables(h, st)
        assert [lh for _, lh in dev] == list(F.heights(st.shape))
        for (buf, lh), w in zip(dev, want):
            got = buf.to_host().reshape(w.shape)
            assert np.array_equal(got, w), np.argwhere(got != w)[:8]
    finally:
        o.oracle_set_params()
        h.close()


@pytest.mark.parametrize("pset", PS.PROVE_SETS)
def test_gpu_proves_the_statement_under_parameter_sets(pset):
    """the statement proven from device tables at the case's own small query count, interpreted and compiled"""
    h = hal.HipHal(0)
    try:
        blob, tables, init, pf = shard(h, PS.PROVE_CASE, pset)
        st = F.statement(tables, pf, init, blob)
        dev = F.device_tables(h, st)
        host = F.host_tables(st)
        got = F.prove(h, st, dev)
        assert np.array_equal(got, o.oracle_p3_prove(host, st.init))
        assert p3.verify(host, got, st.init, params=blob) == 0
        assert F.verify_fri_statement(tables, pf, init, got, blob) == 0
        for air in F.airs(st):
            air.compile(h)
        again = F.prove(h, st, dev)
        assert np.array_equal(again, got)
        assert p3.verify(host, again, st.init, params=blob) == 0 and F.verify_fri_statement(tables, pf, init, again, blob) == 0
    finally:
        o.oracle_set_params()
        h.close()


def test_gpu_proves_the_statement_from_device_tables():
    """SP1's 100 queries over a 2^11-row shard: 6600 path rows, 7700 chip rows"""
    h = hal.HipHal(0)
    try:
        blob, tables, init, pf = shard(h, "sp1_tiny_beside_tall", queries=100)
        st = F.statement(tables, pf, init, blob)
        sz = F.sizes(st.shape)
        assert sz["path_rows"] >= 1 << 12 and sz["chip_rows"] == sz["path_rows"] + sz["fold_rows"]
        dev = F.device_tables(h, st)
        host = F.host_tables(st)
        for (buf, lh), t in zip(dev, host):
            assert np.array_equal(buf.to_host().reshape(t.trace.shape), t.trace)
        got = F.prove(h, st, dev)
        assert np.array_equal(got, o.oracle_p3_prove(host, st.init))
        assert p3.verify(host, got, st.init, params=blob) == 0
        assert F.verify_fri_statement(tables, pf, init, got, blob) == 0
        for air in F.airs(st):
            air.compile(h)
        assert np.array_equal(F.prove(h, st, dev), got)
        assert np.array_equal(F.prove(h, st), got)                 # rows written anew
    finally:
        o.oracle_set_params()
        h.close()


def test_gpu_undersized_buffer_is_refused_with_nothing_written():
    h = hal.HipHal(0)
    try:
        blob, tables, init, pf = shard(h, "sp1_mixed_fib8_cubic4")
        st = F.statement(tables, pf, init, blob)
        sz = F.sizes(st.shape)
        names = ("fold", "path", "claims", "chip")
        words = [sz[n + "_width"] << sz[n + "_log_height"] for n in names]
        mark = [np.full(w, 0x5A5A5A5A, dtype=np.uint32) for w in words]
        bufs = [h.copy_from_elem(m) for m in mark]
        d_pub, d_rec = h.copy_from_elem(st.publics), h.copy_from_elem(st.records)
        lib = _lib.load()
        sh = st.shape
        for short in range(4):
            args = []
            for k, b in enumerate(bufs):
                args += [_ptr(b), words[k] - (1 if k == short else 0)]
            rc = lib.rk_fri_chip_rows_device(h._ctx, sh.log_max, sh.blowup_log2, sh.queries, _ptr(d_pub), _ptr(d_rec), *args)
            assert rc == _lib.RK_ERR_CAPACITY
        h.sync()
        for b, m in zip(bufs, mark):
            assert np.array_equal(b.to_host(), m)
        args = []
        for k, b in enumerate(bufs):
            args += [_ptr(b), words[k]]
        assert lib.rk_fri_chip_rows_device(h._ctx, sh.log_max, sh.blowup_log2 + 1, sh.queries, _ptr(d_pub), _ptr(d_rec), *args) == -1   # not the context's blow-up
        assert lib.rk_fri_chip_rows_device(h._ctx, sh.log_max, sh.blowup_log2, sh.queries, None, _ptr(d_rec), *args) == -1
        assert lib.rk_fri_chip_rows_device(h._ctx, sh.log_max, sh.blowup_log2, sh.queries, _ptr(d_pub), _ptr(d_rec), *args) == 0
        h.sync()
        for b, w in zip(bufs, F.witness(st)):
            assert np.array_equal(b.to_host().reshape(w.shape), p3.to_mont(w))
        h.set_params(0)                                               # the width-24 instance: outside the scope
        assert lib.rk_fri_chip_rows_device(h._ctx, sh.log_max, 2, sh.queries, _ptr(d_pub), _ptr(d_rec), *args) == -1
    finally:
        o.oracle_set_params()
        h.close()
