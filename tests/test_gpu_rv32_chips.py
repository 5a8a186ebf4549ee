"""The rv32i chip set on the GPU: rk_exec_rv32_shard_device's tables against the numpy reference (p3_rv32_shards), word
for word; proofs against the CPU oracle; the whole run verified and chained; forged tables refused with the expected
reasons."""
import numpy as np
import pytest

import oracle_lib as o
import rv32_chip_programs as RP
from raiko_amd import _lib, p3, rv32
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


def device_shards(hal, elf, po2, ext_w):
    airs = X.p3_rv32_airs(ext_w)
    ex, shards, dev, bufs = X.execute_rv32_device(hal, elf, INPUT, po2, airs=airs)
    hal.sync()
    host = []
    for (tables, init), d in zip(shards, bufs):
        host.append([b.to_host().reshape(1 << lg, t.air.width) for (b, lg), t in zip(d, tables)])
    return ex, shards, dev, bufs, host, airs


def free(bufs):
    for d in bufs:
        for b, _ in d:
            b.free()


@pytest.mark.parametrize("po2,loops", [(13, 1), (13, 200), (16, 1500)])
def test_device_tables_equal_numpy(hal, po2, loops):
    """one shard, several shards with a partial last one, a 2^16 shard: every device-written table = the numpy one"""
    elf = RP.alu_program(loops)
    ex, shards, dev, bufs, host, airs = device_shards(hal, elf, po2, p3.EXT_W)
    try:
        ref_ex = X.execute(elf, INPUT, segment_limit_po2=po2, record_trace=True)
        ref = X.p3_rv32_shards(ref_ex, airs=airs)
        assert len(ref) == len(shards)
        if loops > 1:
            assert len(ref) > 1 and ref_ex.segments[-1].cycles < 1 << ref_ex.segments[-1].po2
        for k, ((rt, rinit), got, (tables, init)) in enumerate(zip(ref, host, shards)):
            assert np.array_equal(init, rinit)
            for i, (r, g) in enumerate(zip(rt, got)):
                assert g.shape == r.trace.shape, (k, i)
                bad = np.nonzero(g != r.trace)
                assert bad[0].size == 0, "shard %d table %d: first difference at row %d col %d" % (k, i, bad[0][0], bad[1][0])
                assert np.array_equal(tables[i].public_values, r.public_values)
    finally:
        free(bufs)


def test_proof_words_equal_oracle_and_run_verifies(hal):
    """a 2^13-cycle shard: proof words = or_p3_prove's; the run verifies under verify_rv32_execution; a changed public
    end register breaks the chain"""
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    elf = RP.alu_program(200)
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    shards = X.p3_rv32_shards(ex)
    assert len(shards) >= 2
    tables, init = shards[0]
    got = p3.prove(hal, tables, init)
    assert np.array_equal(got, o.oracle_p3_prove(tables, init))
    proofs = p3.prove_shards(shards, blob, batch=2, verify=True)
    assert np.array_equal(proofs[0], got)
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc)
    # shard 0 claims a different final a0: its proof does not verify against that statement, and the chain of the
    # public values breaks at shard 1
    pub = p3.from_mont(tables[2].public_values).astype(np.int64)
    pub[64 + 2 * 10] ^= 1
    forged = list(tables)
    forged[2] = p3.Table(tables[2].air, tables[2].trace, p3.to_mont(pub))
    with pytest.raises(ValueError, match="shard 0: the proof does not verify"):
        X.verify_rv32_execution([(forged, init)] + shards[1:], proofs, blob)
    publics = X.rv32_publics(shards)
    publics[0] = (publics[0][0], pub)
    with pytest.raises(ValueError, match="shard 1: does not start where shard 0 ended"):
        X.check_rv32_chain(publics)


def forgeries(tables):
    """(name, forged tables, expected rk_p3_verify reason)"""
    canon = RP.tables_canon(tables)
    cpu = canon[0]
    out = []
    rows = lambda sel: np.nonzero(sel)[0]
    # an ADD result off by one, its RANGE16 counts moved along: only the ALU constraint catches it
    r = rows((cpu[:, rv32.IS_ADD] == 1) & (cpu[:, rv32.WR] == 0) & (cpu[:, rv32.RES_LO] < 0xFFFF))[0]
    c = cpu.copy()
    rng = canon[4].copy()
    rng[c[r, rv32.RES_LO], 1] -= 1
    c[r, rv32.RES_LO] += 1
    rng[c[r, rv32.RES_LO], 1] += 1
    out.append(("add", RP.replace(RP.replace(tables, 0, c), 4, rng), 3))
    # an XOR result byte: the BYTE bus
    r = rows((cpu[:, rv32.IS_BIT] == 1) & (cpu[:, rv32.BOP] == 3))[0]
    c = cpu.copy()
    c[r, rv32.BR] ^= 1
    c[r, rv32.RES_LO] ^= 1
    out.append(("xor", RP.replace(tables, 0, c), 8))
    # an rs1 value of a register written earlier in the shard: the REGISTER bus
    r = rows((cpu[:, rv32.PA_TS] > 0) & (cpu[:, rv32.IS_ADD] == 0) & (cpu[:, rv32.IS_BIT] == 0) & (cpu[:, rv32.IS_SLT] == 0)
             & (cpu[:, rv32.IS_SUB] == 0) & (cpu[:, rv32.IS_SLTU] == 0) & (cpu[:, rv32.RS1] != 0))[0]
    c = cpu.copy()
    c[r, rv32.A_LO] ^= 4
    c[r, rv32.SA_CHK] = 2 * c[r, rv32.A_HI] - 65536 * c[r, rv32.SA]
    out.append(("rs1", RP.replace(tables, 0, c), 8))
    # a prev_ts equal to ts: the RANGE16 bus
    r = rows(cpu[:, rv32.PA_TS] > 0)[0]
    c = cpu.copy()
    c[r, rv32.PA_TS] = c[r, rv32.TSA]
    d = (-1) % p3.P
    c[r, rv32.DA_LO], c[r, rv32.DA_HI] = d % 16384, d // 16384
    out.append(("prev_ts", RP.replace(tables, 0, c), 8))
    # a decoded rd index: the PROGRAM bus
    r = rows(cpu[:, rv32.WR] == 1)[0]
    c = cpu.copy()
    c[r, rv32.WREG] = (c[r, rv32.WREG] % 31) + 1
    out.append(("rd", RP.replace(tables, 0, c), 8))
    # a register table initial value that differs from its public value
    pub = p3.from_mont(tables[2].public_values).astype(np.int64)
    pub[2 * 5] ^= 1
    forged = list(tables)
    forged[2] = p3.Table(tables[2].air, tables[2].trace, p3.to_mont(pub))
    out.append(("init", forged, 3))
    return out


def test_forgeries_refused(hal):
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    elf = RP.alu_program(200)
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    shards = X.p3_rv32_shards(ex)
    tables, init = shards[1]
    for name, forged, reason in forgeries(tables):
        pf = p3.prove(hal, forged, init)
        assert p3.verify(forged, pf, init, params=blob) == reason, name
        with pytest.raises(_lib.RkError, match="shard 1") as ei:
            p3.prove_shards([shards[0], (forged, init)], blob, batch=2, verify=True)
        assert ei.value.segment == 1, name


@pytest.mark.parametrize("preset", [0, 1])
def test_execute_and_prove_rv32i(hal, preset):
    """the public entry point, device tables, under both parameter sets: proofs = the host-table route's"""
    blob = H.make_params(preset, **FAST)
    elf = RP.alu_program(200)
    ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=13, params=blob, batch=2, chips="rv32i")
    assert len(proofs) == len(ex.segments) >= 2
    ref = X.p3_rv32_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True), ext_w=int(blob.ext_w))
    ref_proofs = p3.prove_shards(ref, blob, batch=2, verify=True)
    for a, b in zip(proofs, ref_proofs):
        assert np.array_equal(a, b)


def test_padding_row_forgery_refused(hal):
    """x3 = 0xFE forged for xor x3, x1, x2 (0x0F ^ 0xF0), its BYTE lookup cancelled by IS_BIT = -1 on the padding row:
    the buses balance, the proof is refused for the constraint (reason 3), and prove_shards names the shard"""
    import rv32_padding_forgery as F
    blob = hal.set_params(1, **FAST)
    o.oracle_set_params(1, **FAST)
    airs = X.p3_rv32_airs()
    init = np.zeros(16, dtype=np.uint32)
    shards = []
    for build in (F.honest, F.forged):
        canon, pub_cpu, pub_reg = build()
        pubs = [pub_cpu, (), pub_reg, (), ()]
        shards.append(([p3.Table.from_canonical(a, t, pv) for a, t, pv in zip(airs, canon, pubs)], init))
    good = p3.prove(hal, *shards[0])
    assert p3.verify(shards[0][0], good, init, params=blob) == 0
    bad = p3.prove(hal, *shards[1])
    assert np.array_equal(bad, o.oracle_p3_prove(*shards[1]))
    assert p3.verify(shards[1][0], bad, init, params=blob) == 3
    with pytest.raises(_lib.RkError, match="shard 1") as ei:
        p3.prove_shards(shards, blob, batch=2, verify=True)
    assert ei.value.segment == 1


def test_pipeline_rv32i_equals_host_route(hal):
    """P3Pipeline(chips="rv32i"): tables written on the GPU while the executor runs, proofs = the host-table route's,
    the run checked; keep_tables gives back the tables the proofs are of"""
    blob = H.make_params(1, **FAST)
    elf = RP.alu_program(200)
    ex, proofs, kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=13, params=blob, chips="rv32i", keep_tables=True)
    ref = X.p3_rv32_shards(X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True), ext_w=int(blob.ext_w))
    ref_proofs = p3.prove_shards(ref, blob, batch=2, verify=True)
    assert len(proofs) == len(ref_proofs) == len(ex.segments) >= 2
    for a, b in zip(proofs, ref_proofs):
        assert np.array_equal(a, b)
    for (tables, init), (rt, rinit) in zip(kept, ref):
        assert np.array_equal(init, rinit)
        for t, r in zip(tables, rt):
            assert np.array_equal(t.trace, r.trace)
    assert X.verify_rv32_execution(kept, proofs, blob, entry_pc=ex.segments[0].start_pc)
