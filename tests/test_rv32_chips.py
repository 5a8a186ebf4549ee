"""The rv32i chip set on the CPU (raiko_amd/rv32.py, executor.p3_rv32_*): the numpy tables against oracle/or_rv32.py's
execution row by row, every AIR satisfied and every bus balanced on honest tables, each forgery caught by the named
constraint or bus, the chain check over the public values."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import or_rv32  # noqa: E402
import rv32_cf_programs as CP  # noqa: E402
import rv32_chip_programs as RP  # noqa: E402
import rv32_m_programs as MP  # noqa: E402
from raiko_amd import p3, rv32  # noqa: E402
from raiko_amd import executor as X  # noqa: E402

INPUT = [11, 22, 33, 44]


@pytest.fixture(scope="module")
def run():
    elf = RP.alu_program(200)
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    airs = X.p3_rv32_airs()
    shards = X.p3_rv32_shards(ex, airs=airs)
    return elf, ex, airs, shards


def test_airs_shape():
    for a in X.p3_rv32_airs():
        assert a.log_quotient_degree() <= 1
        cols = {c for it in a.interactions for c in it.value_cols + ([] if it.mult_is_const else [it.mult])}
        assert len(cols) <= 120 and all(len(it.value_cols) <= 64 for it in a.interactions)
        a.handle()                                 # rk_air_create_lookup accepts it
    cpu, prog, reg, byte, _ = X.p3_rv32_airs()
    assert (cpu.width, prog.width, reg.width, byte.width) == (rv32.CPU_COLS, rv32.PROGRAM_COLS, rv32.REG_COLS, rv32.BYTE_COLS)


def test_tables_follow_the_oracle(run):
    """register values and per-register access order, row by row, against or_rv32's execution"""
    elf, ex, _airs, shards = run
    want = or_rv32.run(elf, INPUT, segment_limit_po2=13, trace=True)
    assert len(want["traces"]) == len(shards) >= 2
    regs = [0] * 32
    for (tables, _init), rows in zip(shards, want["traces"]):
        cpu = RP.tables_canon(tables)[0]
        start = list(regs)
        last = [0] * 32
        for i, (pc, ins, a, b, res, _nx, wr) in enumerate(rows):
            r = cpu[i]
            assert int(r[rv32.PC_LO] | r[rv32.PC_HI] << 16) == pc
            assert int(r[rv32.A_LO] | r[rv32.A_HI] << 16) == a == regs[(ins >> 15) & 31]
            assert int(r[rv32.B_LO] | r[rv32.B_HI] << 16) == b == regs[(ins >> 20) & 31]
            ecall = ins == 0x73
            rd = 10 if ecall else (ins >> 7) & 31
            assert r[rv32.WR] == (1 if (wr or ecall) else 0)
            ts = 3 * i + 1
            rs1, rs2 = (ins >> 15) & 31, (ins >> 20) & 31
            assert r[rv32.PA_TS] == last[rs1]
            last[rs1] = ts
            assert r[rv32.PB_TS] == last[rs2]
            last[rs2] = ts + 1
            if r[rv32.WR]:
                assert r[rv32.PW_TS] == last[rd]
                assert int(r[rv32.PW_LO] | r[rv32.PW_HI] << 16) == regs[rd]
                last[rd] = ts + 2
                val = int(r[rv32.RES_LO] | r[rv32.RES_HI] << 16)
                if wr:
                    assert val == res
                regs[rd] = val
        assert not cpu[len(rows):, rv32.ACTIVE].any()
        pub = p3.from_mont(tables[2].public_values).astype(np.int64)
        assert [int(pub[2 * j] | pub[2 * j + 1] << 16) for j in range(32)] == start
        assert [int(pub[64 + 2 * j] | pub[65 + 2 * j] << 16) for j in range(32)] == regs
    assert regs == list(want["machine"].x)


def test_honest_tables_satisfy_every_air_and_bus(run):
    _elf, _ex, airs, shards = run
    for k, (tables, _init) in enumerate(shards):
        canon = RP.tables_canon(tables)
        pubs = [p3.from_mont(t.public_values) for t in tables]
        for i in (0, 1, 2):
            assert airs[i].check_trace(canon[i], pubs[i]) == [], (k, i)
        byte = canon[3]
        rows = np.concatenate([np.arange(0, 3 << 16, 4099), np.nonzero(byte[:, rv32.Y_MULT])[0], [(3 << 16) + 7]])
        # check_trace wraps rows around: a sample of rows is a trace of its own (the byte AIR has no transitions)
        sample = byte[np.unique(rows)]
        pad = 1 << int(len(sample) - 1).bit_length()
        sample = np.concatenate([sample, np.zeros((pad - len(sample), rv32.BYTE_COLS), dtype=np.int64)])
        assert airs[3].check_trace(sample) == []
        bal = rv32.bus_balance(canon, airs)
        assert set(bal) == {rv32.BUS_PROGRAM, rv32.BUS_RANGE16, rv32.BUS_REGISTER, rv32.BUS_BYTE}
        assert all(v == {} for v in bal.values()), k


def _violations(air, table, pub=()):
    return air.check_trace(table, pub)


def test_forgeries_caught(run):
    """each forgery breaks the named constraint or the balance of the named bus"""
    _elf, _ex, airs, shards = run
    tables, _init = shards[1]
    canon = RP.tables_canon(tables)
    cpu = canon[0]
    pubs = [p3.from_mont(t.public_values) for t in tables]

    def bus_off(tabs):
        return {b for b, v in rv32.bus_balance(tabs, airs).items() if v}

    # an ADD result off by one with RANGE16 rebalanced: only the ALU constraint
    r = np.nonzero((cpu[:, rv32.IS_ADD] == 1) & (cpu[:, rv32.WR] == 0) & (cpu[:, rv32.RES_LO] < 0xFFFF))[0][0]
    c, rng = cpu.copy(), canon[4].copy()
    rng[c[r, rv32.RES_LO], 1] -= 1
    c[r, rv32.RES_LO] += 1
    rng[c[r, rv32.RES_LO], 1] += 1
    assert bus_off([c] + canon[1:4] + [rng]) == set()
    assert {row for row, _ in _violations(airs[0], c, pubs[0])} == {r}
    # an XOR result byte: the BYTE bus
    r = np.nonzero((cpu[:, rv32.IS_BIT] == 1) & (cpu[:, rv32.BOP] == 3))[0][0]
    c = cpu.copy()
    c[r, rv32.BR] ^= 1
    assert rv32.BUS_BYTE in bus_off([c] + canon[1:])
    # an rs1 value of a register written earlier in the shard: the REGISTER bus
    r = np.nonzero((cpu[:, rv32.PA_TS] > 3 * 0) & (cpu[:, rv32.RS1] != 0) & (cpu[:, rv32.WR] == 1))[0][0]
    c = cpu.copy()
    c[r, rv32.A_LO] ^= 4
    assert rv32.BUS_REGISTER in bus_off([c] + canon[1:])
    # a prev_ts equal to ts: the RANGE16 bus (ts - prev_ts - 1 = p - 1 has no 16-bit limbs)
    r = np.nonzero(cpu[:, rv32.PA_TS] > 0)[0][0]
    c = cpu.copy()
    c[r, rv32.PA_TS] = c[r, rv32.TSA]
    c[r, rv32.DA_LO], c[r, rv32.DA_HI] = (p3.P - 1) % 16384, (p3.P - 1) // 16384
    assert rv32.BUS_RANGE16 in bus_off([c] + canon[1:])
    # a decoded rd index: the PROGRAM bus
    r = np.nonzero(cpu[:, rv32.WR] == 1)[0][0]
    c = cpu.copy()
    c[r, rv32.WREG] = c[r, rv32.WREG] % 31 + 1
    assert rv32.BUS_PROGRAM in bus_off([c] + canon[1:])
    # a program row whose decoded rd is not the word's: the program AIR
    p = canon[1].copy()
    p[0, 6] += 1
    assert _violations(airs[1], p)
    # a register table initial value that differs from its public value
    pub = pubs[2].astype(np.int64).copy()
    pub[2 * 5] ^= 1
    assert _violations(airs[2], canon[2], pub)


def test_chain_check(run):
    _elf, ex, _airs, shards = run
    publics = X.rv32_publics(shards)
    assert X.check_rv32_chain(publics, entry_pc=ex.segments[0].start_pc)
    with pytest.raises(ValueError, match="entry point"):
        X.check_rv32_chain(publics, entry_pc=ex.segments[0].start_pc + 4)
    bad = [(publics[0][0], publics[0][1].astype(np.int64).copy())] + publics[1:]
    bad[0][1][64 + 2 * 10] ^= 1
    with pytest.raises(ValueError, match="shard 1: does not start where shard 0 ended"):
        X.check_rv32_chain(bad)
    bad = [(publics[0][0], publics[0][1].astype(np.int64).copy())] + publics[1:]
    bad[0][1][2 * 3] = 1
    with pytest.raises(ValueError, match="shard 0: the registers do not start at zero"):
        X.check_rv32_chain(bad)


def test_side_data(run):
    """the executor's registers at segment boundaries and its ecall side list (rk_exec_registers / rk_exec_ecalls)"""
    _elf, ex, _airs, _shards = run
    for k, (start, end, ec) in enumerate(ex.rv32):
        if k:
            assert np.array_equal(start, ex.rv32[k - 1][1])
        else:
            assert not start.any()
    ec0 = ex.rv32[0][2]
    assert ec0.shape[0] >= 1 and ec0[0, 1] == 4        # the READ took four words: a0 = 4
    assert ex.rv32[-1][2][-1, 1] == 7                   # the halt leaves a0 = exit code


def test_padding_rows_cannot_cancel_lookups():
    """a padding row whose IS_BIT or IS_SLT is -1 would receive what an active row sends (a forged XOR result, an
    out-of-range limb): every bus balances, and the cpu AIR refuses the padding row"""
    import rv32_padding_forgery as F
    airs = X.p3_rv32_airs()
    for build in (F.honest, F.forged, F.slt_padding):
        tables, pub_cpu, pub_reg = build()
        assert all(v == {} for v in rv32.bus_balance(tables, airs).values()), build.__name__
        assert airs[1].check_trace(tables[1]) == [] and airs[2].check_trace(tables[2], pub_reg) == []
        bad = airs[0].check_trace(tables[0], pub_cpu)
        assert bad == [] if build is F.honest else [row for row, _ in bad] == [1], build.__name__
    tables, _pc, pub_reg = F.forged()
    assert tables[0][0, rv32.RES_LO] == 0xFE and pub_reg[64 + 2 * 3] == 0xFE


# ---- the lane bodies the GPU writes the tables with (raiko_amd/csrc/rv32_rows.hpp), walked over a trace on the CPU
_ROWS_SETS = {"rv32i": 0, "rv32i-cf": 1, "rv32im": 2}
_ROWS_PROGRAMS = {"alu1": lambda: RP.alu_program(1), "cf1": lambda: CP.cf_program(1), "m1": lambda: MP.m_program(1),
                  "mixed400": lambda: MP.mixed_program(400), "alu200": lambda: RP.alu_program(200)}
_ROWS_CASES = [(p, c) for p in ("alu1", "cf1", "m1", "mixed400") for c in _ROWS_SETS] + [("alu200", "rv32im")]
_rows_runs = {}


@pytest.fixture(scope="module")
def rows_lib(tmp_path_factory):
    import ctypes
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("emul_rv32_rows") / "libemul_rv32_rows.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(root, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(root, "tests", "emul", "emul_rv32_rows.cpp")], check=True, capture_output=True)
    return ctypes.CDLL(so)


@pytest.mark.parametrize("program,chips", _ROWS_CASES)
def test_row_bodies_write_the_numpy_tables(rows_lib, program, chips):
    """tests/emul/emul_rv32_rows.cpp walks each segment's trace in order through rv32_rows.hpp's bodies, the last access
    per register kept in an array: its cpu and program tables, and the muldiv table under rv32im, are the chip set's
    shard_tables word for word in Montgomery form.  Segments of 2^13: alu200 and mixed400 end in a partial segment and
    start their later ones from non-zero registers"""
    import ctypes as C
    if program not in _rows_runs:                         # one execution per program, shared by the chip sets
        _rows_runs[program] = X.execute(_ROWS_PROGRAMS[program](), INPUT, segment_limit_po2=13, record_trace=True)
    ex = _rows_runs[program]
    module = X._rv32_set(chips)[0]
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p)
    assert len(ex.segments) >= (2 if program in ("alu200", "mixed400") else 1)
    for s, (_code, data), (start, end, ecalls) in zip(ex.segments, ex.witness, ex.rv32):
        compared = (0, 1, 6) if chips == "rv32im" else (0, 1)           # cpu, program, muldiv
        canon = module.shard_tables(s, data, start, end, ecalls)[0]
        want = {k: p3.to_mont(canon[k]) for k in compared}
        tr, n, pc_lo, pc_hi = rv32.trace_of(s, data)
        rows = np.ascontiguousarray(np.stack([tr[k] for k in ("pc", "ins", "a", "b", "res", "next", "wr")], axis=1), dtype=np.uint32)
        ec = np.ascontiguousarray(ecalls, dtype=np.uint32).reshape(-1, 2)
        init = np.ascontiguousarray(start, dtype=np.uint32)
        got = {k: np.full(w.shape, 0xDEADBEEF, dtype=np.uint32) for k, w in want.items()}
        md = got.get(6, np.zeros((1, 1), dtype=np.uint32))
        rc = rows_lib.emul_rv32_shard(_ROWS_SETS[chips], ptr(rows), C.c_size_t(rows.shape[0]), C.c_size_t(n), C.c_uint32(s.end_pc),
                                      ptr(init), ptr(ec), C.c_size_t(ec.shape[0]), C.c_uint32(pc_lo),
                                      C.c_size_t((pc_hi - pc_lo) // 4 + 1 if rows.shape[0] else 0), C.c_size_t(want[1].shape[0]),
                                      ptr(got[0]), ptr(got[1]), ptr(md), C.c_size_t(md.shape[0]))
        assert rc == 0, (s.index, rc)
        for k in compared:
            assert want[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (s.index, k)
        if s.index and program == "alu200":
            assert start.any()
    assert int(ex.segments[-1].cycles) < 1 << 13
