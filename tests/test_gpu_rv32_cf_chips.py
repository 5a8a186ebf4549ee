"""The rv32i-cf chip set on the GPU: rk_exec_rv32cf_shard_device's tables against the numpy reference
(p3_rv32cf_shards), word for word; proofs against the CPU oracle; the run verified and chained; forged tables refused
with the expected reasons; and the two forgeries rv32i cannot see (a branch taken on a false condition, a wrong SLLI
result) proven and accepted under rv32i, refused under rv32i-cf."""
import numpy as np
import pytest

import oracle_lib as o
import rv32_cf_programs as CP
import rv32_chip_programs as RP
from raiko_amd import _lib, p3, rv32, rv32cf
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


@pytest.mark.parametrize("po2,loops", [(13, 1), (13, 100), (16, 700)])
def test_device_tables_equal_numpy(hal, po2, loops):
    """one shard, several shards with a partial last one, a 2^16 shard: every device-written table = the numpy one"""
    elf = CP.cf_program(loops)
    airs = X.p3_rv32cf_airs()
    ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, po2, airs=airs, chips="rv32i-cf")
    try:
        hal.sync()
        ref_ex = X.execute(elf, INPUT, segment_limit_po2=po2, record_trace=True)
        ref = X.p3_rv32cf_shards(ref_ex, airs=airs)
        assert len(ref) == len(shards) == len(bufs)
        if loops > 1:
            assert len(ref) > 1 and ref_ex.segments[-1].cycles < 1 << ref_ex.segments[-1].po2
        for k, ((rt, rinit), d, (tables, init)) in enumerate(zip(ref, bufs, shards)):
            assert np.array_equal(init, rinit)
            assert len(d) == 6
            for i, (r, (b, lg), t) in enumerate(zip(rt, d, tables)):
                g = b.to_host().reshape(1 << lg, t.air.width)
                assert g.shape == r.trace.shape, (k, i)
                bad = np.nonzero(g != r.trace)
                assert bad[0].size == 0, "shard %d table %d: first difference at row %d col %d" % (k, i, bad[0][0], bad[1][0])
                assert np.array_equal(t.public_values, r.public_values)
    finally:
        free(bufs)


def test_rv32i_device_tables_unchanged(hal):
    """rk_exec_rv32_shard_device beside the new entry point: rv32i's tables are the cf tables' leading columns"""
    elf = CP.cf_program(100)
    ex, shards, _dev, bufs = X.execute_rv32_device(hal, elf, INPUT, 13, chips="rv32i")
    ref = X.p3_rv32_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True))
    try:
        hal.sync()
        for (rt, _), d, (tables, _) in zip(ref, bufs, shards):
            for r, (b, lg), t in zip(rt, d, tables):
                assert np.array_equal(b.to_host().reshape(1 << lg, t.air.width), r.trace)
    finally:
        free(bufs)


def test_proof_words_equal_oracle_and_run_verifies(hal):
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    elf = CP.cf_program(100)
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    shards = X.p3_rv32cf_shards(ex)
    assert len(shards) >= 3
    tables, init = shards[0]
    got = p3.prove(hal, tables, init)
    assert np.array_equal(got, o.oracle_p3_prove(tables, init))
    proofs = p3.prove_shards(shards, blob, batch=2, verify=True)
    assert np.array_equal(proofs[0], got)
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc)
    # a shift table of another height is refused (reason 2)
    small = rv32cf.shift_rows()[: 1 << 11]
    t5 = p3.Table.from_canonical(tables[5].air, small)
    assert X.verify_rv32_shard(tables[:5] + [t5], p3.prove(hal, tables[:5] + [t5], init), init, blob) == 2


def forgeries(tables):
    """(name, forged tables, expected rk_p3_verify reason)"""
    canon = RP.tables_canon(tables)
    cpu = canon[0]
    out = []
    # an SRA result, the next write of the same register seeing it and RANGE16 moved along: the shift constraint
    for r in np.nonzero((cpu[:, rv32cf.IS_SRA] == 1) & (cpu[:, rv32.WR] == 1))[0]:
        reg = cpu[r, rv32.WREG]
        r2 = r + 1 + np.nonzero((cpu[r + 1:, rv32.WR] == 1) & (cpu[r + 1:, rv32.WREG] == reg))[0][0]
        if not ((cpu[r + 1:r2 + 1, rv32.RS1] == reg) | (cpu[r + 1:r2 + 1, rv32.RS2] == reg)).any():
            break
    else:
        raise AssertionError("no SRA result that is overwritten before it is read")
    c, rng = cpu.copy(), canon[4].copy()
    rng[c[r, rv32.RES_LO], 1] -= 1
    c[r, rv32.RES_LO] ^= 1
    c[r2, rv32.PW_LO] ^= 1
    rng[c[r, rv32.RES_LO], 1] += 1
    out.append(("sra", RP.replace(RP.replace(tables, 0, c), 4, rng), 3))
    r = np.nonzero(cpu[:, rv32cf.IS_SHIFT] == 1)[0][0]                   # a shift-table part: the SHIFT bus
    c = cpu.copy()
    c[r, rv32cf.SLO] ^= 1
    out.append(("shift lookup", RP.replace(tables, 0, c), 8))
    t = canon[5].copy()                                                   # a forged shift-table row: its AIR
    t[3 * 256 + 0x81, rv32cf.H_LO] ^= 1
    out.append(("shift table", RP.replace(tables, 5, t), 3))
    return out


def test_forgeries_refused(hal):
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    ex = X.execute(CP.cf_program(100), INPUT, segment_limit_po2=13, record_trace=True)
    shards = X.p3_rv32cf_shards(ex)
    tables, init = shards[1]
    for name, forged, reason in forgeries(tables):
        pf = p3.prove(hal, forged, init)
        assert p3.verify(forged, pf, init, params=blob) == reason, name
        with pytest.raises(_lib.RkError, match="shard 1") as ei:
            p3.prove_shards([shards[0], (forged, init)], blob, batch=2, verify=True)
        assert ei.value.segment == 1, name


@pytest.mark.parametrize("case", ["BLT_FALSE", "SLLI_WRONG"])
def test_forgery_rv32i_accepts_and_cf_refuses(hal, case):
    """THE GAP: a branch taken on a false condition / a wrong SLLI result proves and verifies under rv32i (reason 0) and
    is refused under rv32i-cf (reason 3, the constraint; prove_shards names the shard)"""
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    init = np.zeros(16, dtype=np.uint32)
    kw = getattr(CP, case)
    for chips, airs, want in (("rv32i", X.p3_rv32_airs(), 0), ("rv32i-cf", X.p3_rv32cf_airs(), 3)):
        canon, pub_cpu, pub_reg = CP.one_row(chips, **kw)
        pubs = [pub_cpu, (), pub_reg, (), (), ()]
        tables = [p3.Table.from_canonical(a, t, pv) for a, t, pv in zip(airs, canon, pubs)]
        pf = p3.prove(hal, tables, init)
        assert np.array_equal(pf, o.oracle_p3_prove(tables, init)), chips
        assert X.verify_rv32_shard(tables, pf, init, blob) == want, chips
        if want:
            honest = CP.one_row(chips, **dict(kw, nxt=0x1004, res=0x80000008))
            good = [p3.Table.from_canonical(a, t, pv) for a, t, pv in zip(airs, honest[0], [honest[1], (), honest[2], (), (), ()])]
            with pytest.raises(_lib.RkError, match="shard 1") as ei:
                p3.prove_shards([(good, init), (tables, init)], blob, batch=2, verify=True)
            assert ei.value.segment == 1


def test_forged_decisions_proven_and_refused(hal):
    """each branch going the way its condition does not, the one-row trace consistent (TAKEN, target, carries, counts):
    rv32i proves and accepts it (reason 0); rv32i-cf's proof equals the oracle's and is refused for the decision
    constraint (reason 3)"""
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    init = np.zeros(16, dtype=np.uint32)
    for op, (a, b) in zip(("beq", "bne", "blt", "bge", "bltu", "bgeu"), CP.BRANCH_EDGES + CP.BRANCH_EDGES[:2]):
        kw = CP.branch_forgery(op, a, b, backward=op in ("bne", "bge"))
        for chips, airs, want in (("rv32i", X.p3_rv32_airs(), 0), ("rv32i-cf", X.p3_rv32cf_airs(), 3)):
            canon, pub_cpu, pub_reg = CP.one_row(chips, **kw)
            tables = [p3.Table.from_canonical(t_air, t, pv) for t_air, t, pv in zip(airs, canon, [pub_cpu, (), pub_reg, (), (), ()])]
            pf = p3.prove(hal, tables, init)
            if want:
                assert np.array_equal(pf, o.oracle_p3_prove(tables, init)), op
            assert X.verify_rv32_shard(tables, pf, init, blob) == want, (op, chips)


@pytest.mark.parametrize("preset", [0, 1])
def test_execute_and_prove_rv32cf(hal, preset):
    """the public entry point, device tables, under both parameter sets: proofs = the host-table route's"""
    blob = H.make_params(preset, **FAST)
    elf = CP.cf_program(100)
    ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=13, params=blob, batch=2, chips="rv32i-cf")
    assert len(proofs) == len(ex.segments) >= 3
    ref = X.p3_rv32cf_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True), ext_w=int(blob.ext_w))
    ref_proofs = p3.prove_shards(ref, blob, batch=2, verify=True)
    for a, b in zip(proofs, ref_proofs):
        assert np.array_equal(a, b)


def test_pipeline_rv32cf_equals_host_route(hal):
    blob = H.make_params(1, **FAST)
    elf = CP.cf_program(100)
    ex, proofs, kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=13, params=blob, chips="rv32i-cf",
                                                        keep_tables=True)
    ref = X.p3_rv32cf_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True), ext_w=int(blob.ext_w))
    ref_proofs = p3.prove_shards(ref, blob, batch=2, verify=True)
    assert len(proofs) == len(ref_proofs) == len(ex.segments) >= 3
    for a, b in zip(proofs, ref_proofs):
        assert np.array_equal(a, b)
    for (tables, init), (rt, rinit) in zip(kept, ref):
        assert np.array_equal(init, rinit)
        for t, r in zip(tables, rt):
            assert np.array_equal(t.trace, r.trace)
    assert X.verify_rv32_execution(kept, proofs, blob, entry_pc=ex.segments[0].start_pc)
