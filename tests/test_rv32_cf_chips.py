"""The rv32i-cf chip set on the CPU (raiko_amd/rv32cf.py, executor.p3_rv32cf_*): a strict extension of rv32i's tables,
next pc / branch decisions / shift results against oracle/or_rv32.py's execution row by row, every AIR satisfied and
every bus balanced on honest tables, each forgery caught by the named constraint or bus."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import or_rv32  # noqa: E402
import rv32_cf_programs as CP  # noqa: E402
import rv32_chip_programs as RP  # noqa: E402
from raiko_amd import p3, rv32, rv32cf  # noqa: E402
from raiko_amd import executor as X  # noqa: E402
from raiko_amd.rv32cf import (BD_LO, DROP, IS_BR, IS_JAL, IS_SHIFT, IS_SLL, IS_SRA, IS_SRL, KB, M_SA,  # noqa: E402
                              M_SB, NC0, SK, SX, TAKEN, V_HI, V_LO)

INPUT = [11, 22, 33, 44]


@pytest.fixture(scope="module")
def run():
    elf = CP.cf_program(100)
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    airs = X.p3_rv32cf_airs()
    shards = X.p3_rv32cf_shards(ex, airs=airs)
    return elf, ex, airs, shards


def test_airs_shape():
    airs = X.p3_rv32cf_airs()
    for a in airs:
        assert a.log_quotient_degree() <= 1
        cols = {c for it in a.interactions for c in it.value_cols + ([] if it.mult_is_const else [it.mult])}
        assert len(cols) <= 120 and all(len(it.value_cols) <= 64 for it in a.interactions)
        a.handle()
    assert [a.width for a in airs] == [rv32cf.CPU_COLS, rv32cf.PROGRAM_COLS, rv32.REG_COLS, rv32.BYTE_COLS, 2,
                                       rv32cf.SHIFT_COLS]
    assert rv32cf.BUS_SHIFT not in (rv32.BUS_PROGRAM, rv32.BUS_RANGE16, 4, rv32.BUS_REGISTER, rv32.BUS_BYTE)
    # rv32i's AIRs are untouched and p3_rv32_airs still gives them
    assert [a.width for a in X.p3_rv32_airs()] == [rv32.CPU_COLS, rv32.PROGRAM_COLS, rv32.REG_COLS, rv32.BYTE_COLS, 2]


def test_strict_extension_of_rv32i(run):
    """cpu columns 0..67, program columns 0..76 and the register / byte tables are rv32i's on the same execution"""
    _elf, ex, _airs, shards = run
    ref = X.p3_rv32_shards(ex)
    assert len(ref) == len(shards) >= 3
    for (cf, _), (ri, _) in zip(shards, ref):
        c, r = RP.tables_canon(cf), RP.tables_canon(ri)
        assert np.array_equal(c[0][:, :rv32.CPU_COLS], r[0])
        assert np.array_equal(c[1][:, :rv32.PROGRAM_COLS], r[1])
        assert np.array_equal(c[2], r[2]) and np.array_equal(c[3], r[3])
        assert (c[4][:, 1] >= r[4][:, 1]).all()             # the range counts grow by the new sends only
        assert np.array_equal(cf[0].public_values, ri[0].public_values)
        assert np.array_equal(cf[2].public_values, ri[2].public_values)


def test_rows_follow_the_oracle(run):
    """next pc, TAKEN and every written shift result against or_rv32's execution, row by row"""
    elf, _ex, _airs, shards = run
    want = or_rv32.run(elf, INPUT, segment_limit_po2=13, trace=True)
    assert len(want["traces"]) == len(shards)
    seen = set()
    for (tables, _init), rows in zip(shards, want["traces"]):
        cpu = RP.tables_canon(tables)[0]
        for i, (pc, ins, a, b, res, nx, wr) in enumerate(rows):
            r = cpu[i]
            assert int(r[rv32.NX_LO] | r[rv32.NX_HI] << 16) == nx
            op, f3 = ins & 0x7F, (ins >> 12) & 7
            if op == 0x63:
                sa, sb = a - (a >> 31 << 32), b - (b >> 31 << 32)
                cond = {0: a == b, 1: a != b, 4: sa < sb, 5: sa >= sb, 6: a < b, 7: a >= b}[f3]
                assert r[TAKEN] == int(cond) and r[IS_BR] == 1
                assert nx == ((pc + (r[rv32cf.JIMM_LO] | r[rv32cf.JIMM_HI] << 16)) & 0xFFFFFFFF if cond else pc + 4)
                seen.add((f3, bool(cond), nx < pc))
            else:
                assert r[TAKEN] == 0 and r[IS_BR] == 0
            if op in (0x13, 0x33) and f3 in (1, 5) and not (op == 0x33 and ins >> 25 == 1):
                assert r[IS_SHIFT] == 1
                if wr:
                    assert int(r[V_LO] | r[V_HI] << 16) == res == int(r[rv32.RES_LO] | r[rv32.RES_HI] << 16)
            else:
                assert r[IS_SHIFT] == 0
            if op == 0x67:
                seen.add(("jalr", int(r[DROP])))
    for f3 in (0, 1, 4, 5, 6, 7):
        assert {(f3, True), (f3, False)} <= {k[:2] for k in seen if k[0] == f3}, f3
        assert (f3, True, True) in seen                          # a backward target taken
    assert ("jalr", 1) in seen and ("jalr", 0) in seen


def test_honest_tables_satisfy_every_air_and_bus(run):
    _elf, _ex, airs, shards = run
    for k, (tables, _init) in enumerate(shards):
        canon = RP.tables_canon(tables)
        bal = rv32.bus_balance(canon, airs)
        assert set(bal) == {rv32.BUS_PROGRAM, rv32.BUS_RANGE16, rv32.BUS_REGISTER, rv32.BUS_BYTE, rv32cf.BUS_SHIFT}
        assert all(v == {} for v in bal.values()), k
    canon = RP.tables_canon(shards[-1][0])                  # the partial last shard: the AIRs row by row
    pubs = [p3.from_mont(t.public_values) for t in shards[-1][0]]
    for i in (0, 1, 2, 5):
        assert airs[i].check_trace(canon[i], pubs[i]) == [], i
    assert canon[0][:, rv32.ACTIVE].sum() < canon[0].shape[0]


@pytest.fixture(scope="module")
def small():
    """one pass in a shard of 256 rows (the executed 2^13-row segment cut short), small enough to check every AIR row by
    row after each forgery"""
    ex = X.execute(CP.cf_program(1), INPUT, segment_limit_po2=13, record_trace=True)
    seg, (start, end, ecalls) = ex.segments[0], ex.rv32[0]
    assert len(ex.segments) == 1 and 128 < seg.cycles < 256
    canon, pub_cpu, pub_reg = rv32cf.shard_tables(seg, ex.witness[0][1][:, :256], start, end, ecalls)
    return X.p3_rv32cf_airs(), canon, [pub_cpu, (), pub_reg, (), (), ()]


def _caught(airs, canon, pubs, k, t, bus=None):
    """table k replaced by t: the rows the AIR refuses, or the buses that no longer balance"""
    tabs = list(canon)
    tabs[k] = t
    if bus is not None:
        return {b for b, v in rv32.bus_balance(tabs, airs).items() if v}
    return {row for row, _ in airs[k].check_trace(t, pubs[k])}


def _refused(air, tables, pub):
    """the (row, constraint name) pairs the cpu AIR refuses; rv32i's own constraints by index"""
    inv = {k: n for n, k in air.constraint_names.items()}
    return {(row, inv.get(k, k)) for row, k in air.check_trace(tables[0], pub)}


def _buses_off(airs, tables):
    return {b for b, v in rv32.bus_balance(tables, airs).items() if v}


def _cf_row(**kw):
    tables, pub_cpu, _pub_reg = CP.one_row("rv32i-cf", **kw)
    return tables, pub_cpu


@pytest.mark.parametrize("op", ["beq", "bne", "blt", "bge", "bltu", "bgeu"])
def test_forged_decisions_refused_by_the_decision_constraint(op):
    """each condition at its edges, going the way it does not, forward and backward, the trace kept consistent (TAKEN,
    target, carries, SEQ / CARRY, the next row's pc, every count): under rv32i every AIR and bus holds it; under rv32i-cf
    every bus balances and the decision constraint alone refuses the row"""
    airs, airs_i = X.p3_rv32cf_airs(), X.p3_rv32_airs()
    for a, b in CP.BRANCH_EDGES:
        for backward in (False, True):
            kw = CP.branch_forgery(op, a, b, backward)
            tables, pub_cpu, pub_reg = CP.one_row("rv32i", **kw)
            assert airs_i[0].check_trace(tables[0], pub_cpu) == [] and not _buses_off(airs_i, tables)
            tables, pub_cpu = _cf_row(**kw)
            assert tables[0][0, TAKEN] == (not CP.condition(op, a, b))
            assert not _buses_off(airs, tables), (op, a, b)
            assert _refused(airs[0], tables, pub_cpu) == {(0, "decision")}, (op, a, b, backward)
            target = kw["pc"] + (-0x40 if backward else 0x40)
            tables, pub_cpu = _cf_row(**dict(kw, nxt=target if kw["nxt"] == kw["pc"] + 4 else kw["pc"] + 4))
            assert _refused(airs[0], tables, pub_cpu) == set()


def test_equality_test_refuses_forged_eq():
    """BEQ / BNE on unequal values with EQ = 1, INV = 0 (the decision then holds): only BD_LO + BD_HI = 0 when EQ refuses
    it; BEQ on equal values with EQ = 0: only the inverse relation refuses it"""
    airs = X.p3_rv32cf_airs()
    for op, a, b, eq, want in (("beq", 5, 6, 1, "eq_zero"), ("bne", 0x80000000, 0, 1, "eq_zero"),
                               ("beq", 0x7FFFFFFF, 0x7FFFFFFF, 0, "eq_inv")):
        tables, pub_cpu = _cf_row(**CP.branch_forgery(op, a, b))
        tables[0][0, rv32cf.EQ], tables[0][0, rv32cf.INV] = eq, 0
        assert not _buses_off(airs, tables)
        assert _refused(airs[0], tables, pub_cpu) == {(0, want)}, (op, a, b)


def test_signed_branch_sign_bits_range_checked():
    """BLT on 0x7FFFFFFF, 0x80000000 taken by claiming b's sign bit SB = 0 (SB_CHK = 65536, SNE = 0): every constraint
    holds and only RANGE16 refuses it; with M_SB = 0 as well (SB_CHK then not sent) every bus balances and only M_SB's
    constraint refuses it"""
    airs = X.p3_rv32cf_airs()
    tables, pub_cpu = _cf_row(**CP.branch_forgery("blt", 0x7FFFFFFF, 0x80000000))
    cpu = tables[0]
    cpu[0, rv32.SB], cpu[0, rv32.SNE], cpu[0, rv32.SB_CHK] = 0, 0, 65536
    tables = CP.balance(tables)
    assert _refused(airs[0], tables, pub_cpu) == set()
    assert _buses_off(airs, tables) == {rv32.BUS_RANGE16}
    cpu[0, M_SB] = 0
    tables = CP.balance(tables)
    assert not _buses_off(airs, tables)
    assert _refused(airs[0], tables, pub_cpu) == {(0, "m_sb")}


def _target_off(cpu, r):
    c = cpu.copy()
    c[r, rv32.NX_LO] += 4
    c[r + 1, rv32.PC_LO] += 4                                 # the chain stays intact: only the target is wrong
    c[r, rv32cf.NXH] += 2 * c[r, rv32.IS_LINK]                # and the target's half moves with it
    return c


def _refused_at(air, c, pub, r):
    inv = {k: n for n, k in air.constraint_names.items()}
    return {inv.get(k, k) for row, k in air.check_trace(c, pub) if row == r}


def test_targets_caught(small):
    """a target off by 4 for a taken branch, JAL and JALR: the next-pc constraint on that row; a JALR whose low bit is
    not cleared: the even-target constraint, and with NXH = nx_lo / 2 in the field the RANGE16 bus"""
    airs, canon, pubs = small
    cpu = canon[0]
    jalr = (cpu[:, rv32.IS_LINK] == 1) & (cpu[:, IS_JAL] == 0)
    for name, sel in (("branch", cpu[:, TAKEN] == 1), ("jal", cpu[:, IS_JAL] == 1), ("jalr", jalr)):
        r = np.nonzero(sel & (cpu[:, rv32.NX_LO] < 0xFFF0))[0][0]
        assert _refused_at(airs[0], _target_off(cpu, r), pubs[0], r) == {"next_lo"}, name
    r = np.nonzero(jalr & (cpu[:, DROP] == 1))[0][0]
    c = cpu.copy()
    c[r, rv32.NX_LO] += 1
    c[r + 1, rv32.PC_LO] += 1
    c[r, DROP] = 0
    assert _refused_at(airs[0], c, pubs[0], r) == {"nx_even"}
    c[r, rv32cf.NXH] = c[r, rv32.NX_LO] * pow(2, p3.P - 2, p3.P) % p3.P
    assert _refused_at(airs[0], c, pubs[0], r) == set()      # NXH = nx_lo / 2 in the field holds the row ...
    assert rv32.BUS_RANGE16 in _caught(airs, canon, pubs, 0, c, bus=True)   # ... but is no 16-bit limb


def test_wrong_shift_results_caught(small):
    """a wrong result of each shift, register and immediate form: the result constraint of that row"""
    airs, canon, pubs = small
    cpu = canon[0]
    for name, col in (("sll", IS_SLL), ("srl", IS_SRL), ("sra", IS_SRA)):
        for imm in (0, 1):
            r = np.nonzero((cpu[:, col] == 1) & (cpu[:, rv32.IS_IMM] == imm) & (cpu[:, rv32.WR] == 1))[0][0]
            c = cpu.copy()
            c[r, rv32.RES_LO] ^= 1
            assert _refused_at(airs[0], c, pubs[0], r) == {"result 0"}, (name, imm)
    tables, pub_cpu = _cf_row(**CP.SLLI_WRONG)
    assert not _buses_off(airs, tables) and _refused(airs[0], tables, pub_cpu) == {(0, "result 0")}


def _register_shift(op, a, b, res):
    return dict(ins=CP.A.encode(op, ("x3", "x1", "x2"), 0x1000, {}), a=a, b=b, nxt=0x1004, res=res)


def test_shift_of_32_as_k_8_refused():
    """SRL by a register holding 32 (amount 0) claimed as a shift by 32 written k = 8, q = 3 (result 0): the shift
    lookups, counts and result are consistent, and only k's top bit constraint refuses it"""
    airs = X.p3_rv32cf_airs()
    tables, pub_cpu = _cf_row(**_register_shift("srl", 0x80000001, 32, 0))
    assert CP.set_shift(tables[0], 0, [0, 0, 2], 3, 0) == 0
    tables = CP.balance(tables)
    assert not _buses_off(airs, tables)
    assert _refused(airs[0], tables, pub_cpu) == {(0, "bool %d" % (KB + 2))}


def test_register_amount_quotient_range_checked():
    """SLL / SRL / SRA by a register holding 0x25 (amount 5) claimed as a shift by 6, the quotient T = (0x25 - 6) / 32 in
    the field: every constraint holds and only RANGE16 refuses it (T itself is range-checked, not 32 T)"""
    airs = X.p3_rv32cf_airs()
    for op in ("sll", "srl", "sra"):
        t = (0x25 - 6) * pow(32, p3.P - 2, p3.P) % p3.P
        probe, _ = _cf_row(**_register_shift(op, 0x80000F01, 0x25, 0))
        v = CP.set_shift(probe[0], 0, [0, 1, 1], 0, t)               # the result of a shift by 6
        tables, pub_cpu = _cf_row(**_register_shift(op, 0x80000F01, 0x25, v))
        assert CP.set_shift(tables[0], 0, [0, 1, 1], 0, t) == v
        tables = CP.balance(tables)
        assert _refused(airs[0], tables, pub_cpu) == set(), op
        assert _buses_off(airs, tables) == {rv32.BUS_RANGE16}, op


def test_padding_rows_cannot_hold_multiplicities(small):
    """-1 in each new multiplicity column on a padding row: the cpu AIR refuses that row"""
    airs, canon, pubs = small
    cpu = canon[0]
    pad = int(np.nonzero(cpu[:, rv32.ACTIVE] == 0)[0][1])
    for col in (IS_BR, IS_SHIFT, M_SA, M_SB, rv32.IS_LINK):
        c = cpu.copy()
        c[pad, col] = p3.P - 1
        assert pad in _caught(airs, canon, pubs, 0, c), col


def test_forged_shift_table_row_caught(small):
    airs, canon, pubs = small
    t = canon[5].copy()
    r = 3 * 256 + 0x81                                           # k = 3, x = 0x81: lo = 0x08, hi = 0x04
    assert (t[r, rv32cf.H_LO], t[r, rv32cf.H_HI]) == (0x08, 0x04)
    t[r, rv32cf.H_LO] = 0x09
    assert _caught(airs, canon, pubs, 5, t) == {r}
    t = canon[5].copy()
    t[r, rv32cf.H_K] = 8                                         # the one-hot k says 3
    assert _caught(airs, canon, pubs, 5, t) == {r}


def test_shift_lookups_and_range_sends_balance(small):
    """a changed shift-table lookup or a changed BD limb unbalances the SHIFT / RANGE16 bus"""
    airs, canon, pubs = small
    cpu = canon[0]
    r = np.nonzero(cpu[:, IS_SHIFT] == 1)[0][0]
    c = cpu.copy()
    c[r, SK] += 1
    assert rv32cf.BUS_SHIFT in _caught(airs, canon, pubs, 0, c, bus=True)
    r = np.nonzero(cpu[:, IS_BR] == 1)[0][0]
    c = cpu.copy()
    c[r, BD_LO] += 1
    assert rv32.BUS_RANGE16 in _caught(airs, canon, pubs, 0, c, bus=True)
    assert cpu[:, SX].max() <= 255 and cpu[:, NC0].max() <= 1


@pytest.mark.parametrize("case", ["BLT_FALSE", "SLLI_WRONG"])
def test_hand_built_forgery_only_cf_refuses(case):
    """a taken branch whose condition is false, an SLLI with a wrong result: rv32i's AIRs hold them, rv32i-cf's do not"""
    kw = getattr(CP, case)
    tables, pub_cpu, pub_reg = CP.one_row("rv32i", **kw)
    airs = X.p3_rv32_airs()
    pubs = [pub_cpu, (), pub_reg, (), ()]
    assert all(airs[i].check_trace(tables[i], pubs[i]) == [] for i in (0, 1, 2))
    assert all(v == {} for v in rv32.bus_balance(tables, airs).values())
    tables, pub_cpu, pub_reg = CP.one_row("rv32i-cf", **kw)
    airs = X.p3_rv32cf_airs()
    assert all(v == {} for v in rv32.bus_balance(tables, airs).values())
    want = {(0, "decision")} if case == "BLT_FALSE" else {(0, "result 0")}
    assert tables[0][0, TAKEN] == (case == "BLT_FALSE") and _refused(airs[0], tables, pub_cpu) == want
