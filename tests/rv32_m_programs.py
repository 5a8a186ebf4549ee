"""TEST INFRASTRUCTURE: the guest programs and the hand-built rows of the rv32im chip set tests: all eight M ops on every
pair of edge values (division by zero, -2^31 / -1, rs1 = rs2 among them), an M instruction into x0, a loop long enough
for several 2^13 shards; the Python integer arithmetic the results are checked against; and a one-row shard helper for
the traces an honest executor never writes."""
import numpy as np

import rv32_asm as A
import rv32_cf_programs as CP
from raiko_amd import rv32, rv32cf, rv32im

HALT = A.li("t0", 0) + [("ecall",)]
VALUES = (0, 1, 0xFFFFFFFF, 2, 7, (-7) & 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0x8765F0A1, 0x1234ABCD)
VREGS = ("s0", "s1", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "s9")
M = 0xFFFFFFFF


def _signed(v):
    return v - (v >> 31 << 32)


def m_result(op, a, b):
    """the RISC-V M chapter's result of op ("mul" .. "remu" or its funct3) on 32-bit a, b, in Python integers"""
    op = rv32im.M_OPS[op] if isinstance(op, int) else op
    sa, sb = _signed(a), _signed(b)
    if op == "mul":
        return (a * b) & M
    if op == "mulh":
        return ((sa * sb) >> 32) & M
    if op == "mulhsu":
        return ((sa * b) >> 32) & M
    if op == "mulhu":
        return (a * b) >> 32
    if op in ("divu", "remu"):
        if b == 0:
            return M if op == "divu" else a
        return a // b if op == "divu" else a % b
    if b == 0:
        return M if op == "div" else a
    if sa == -(1 << 31) and sb == -1:
        return a if op == "div" else 0
    q = abs(sa) // abs(sb)
    q = -q if (sa < 0) != (sb < 0) else q
    return q & M if op == "div" else (sa - q * sb) & M


def _m_block(rd_cycle=("a2", "a3", "a4", "a5", "a6", "a7")):
    """every op on every ordered pair of VALUES (the diagonal is rs1 = rs2), rd cycling over six registers"""
    out, k = [], 0
    for op in rv32im.M_OPS:
        for x in VREGS:
            for y in VREGS:
                out.append((op, rd_cycle[k % len(rd_cycle)], x, y))
                k += 1
    return out


def m_program(loops=1):
    """the M cases (800 instructions, then a MUL and a DIV into x0), `loops` passes of them (a backward bne closes the
    loop): almost every row an M row"""
    prog = A.li("t0", 1) + A.li("a0", 0x300100) + [("addi", "a1", "zero", 4), ("ecall",)]
    for r, v in zip(VREGS, VALUES):
        prog += A.li(r, v)
    body = _m_block() + [("mul", "zero", "s8", "s9"), ("div", "zero", "s7", "s2")]
    prog += A.li("tp", loops) + ["loop:"] + body + [("addi", "tp", "tp", -1), ("bne", "tp", "zero", "loop")]
    prog += A.li("a0", 7) + HALT
    code, _ = A.assemble(prog)
    return A.elf(code, data=b"\0" * 0x200)


def mixed_program(loops=1):
    """a loop of ALU work with one M instruction of each kind among it: a few percent of the rows are M rows"""
    body = []
    for k, op in enumerate(rv32im.M_OPS):
        body += [("add", "t1", "t1", "s8"), ("xor", "t2", "t2", "t1"), ("slli", "t3", "t2", 3), ("sub", "t4", "t3", "s9"),
                 ("and", "t5", "t4", "s6"), ("or", "t6", "t5", "s1"), ("addi", "a2", "a2", 1),
                 ("sltu", "a3", "t4", "t1"), (op, "a4", "t1", VREGS[k % len(VREGS)])]
    prog = A.li("t0", 1) + A.li("a0", 0x300100) + [("addi", "a1", "zero", 4), ("ecall",)]
    for r, v in zip(VREGS, VALUES):
        prog += A.li(r, v)
    prog += A.li("tp", loops) + ["loop:"] + body + [("addi", "tp", "tp", -1), ("bne", "tp", "zero", "loop")]
    prog += A.li("a0", 7) + HALT
    code, _ = A.assemble(prog)
    return A.elf(code, data=b"\0" * 0x200)


def one_row(chips, ins, a, b, res, pc=0x1000, md_rows=None):
    """a one-cycle shard of `chips` ("rv32i-cf" or "rv32im") running instruction `ins` at `pc` on rs1 / rs2 values a / b
    and claiming result `res`, every other column filled as an executor that writes that result would fill it: under
    rv32im the muldiv row is the true witness of the op with the claimed result in RES (rv32im.muldiv_rows strict=False);
    md_rows: the muldiv table's height (default the least) -> canonical tables, cpu publics, register publics"""
    if chips == "rv32i-cf":
        return CP.one_row(chips, ins, a, b, pc + 4, res, pc)
    init = np.zeros(32, dtype=np.int64)
    init[(ins >> 15) & 31], init[(ins >> 20) & 31] = a, b
    tr = dict(pc=np.array([pc]), ins=np.array([ins]), a=np.array([a]), b=np.array([b]), res=np.array([res]),
              next=np.array([pc + 4]))
    ec = np.zeros((0, 2), dtype=np.int64)
    cpu, final, final_ts, hist, byte_mult, shift_mult, sends = rv32im.cpu_rows(tr, 2, pc + 4, init, ec, strict=False)
    md, h2, b2, s2 = rv32im.muldiv_rows(sends, md_rows, strict=False)
    prog = rv32im.program_table_for(tr["pc"], tr["ins"], pc, pc)
    tables = [cpu, prog, rv32.register_rows(init, final, final_ts), rv32.byte_rows(byte_mult + b2),
              np.stack([np.arange(1 << 16, dtype=np.int64), hist + h2], axis=1), rv32cf.shift_rows(shift_mult + s2), md]
    pub_cpu = np.array([pc & 0xFFFF, pc >> 16, (pc + 4) & 0xFFFF, (pc + 4) >> 16], dtype=np.int64)
    return tables, pub_cpu, rv32.register_publics(init, final)


def m_ins(op, rd="x3", rs1="x1", rs2="x2"):
    return A.encode(op, (rd, rs1, rs2), 0x1000, {})


# a MUL claiming a wrong low word
MUL_WRONG = dict(ins=m_ins("mul"), a=0x8765F0A1, b=0x1234ABCD, res=(0x8765F0A1 * 0x1234ABCD + 1) & M)


def balance(tables):
    """an rv32im shard's range, byte and shift counts recomputed from what its cpu and muldiv tables send, as a forger
    who edited cells would: only values those tables hold can be counted"""
    from raiko_amd.segment import P
    tables = CP.balance(tables[:6]) + list(tables[6:])
    md = np.asarray(tables[6], dtype=np.int64) % P
    rng, byte, sh = tables[4].copy(), tables[3].copy(), tables[5].copy()
    on = md[:, rv32im.D_MULT]
    for c in rv32im.RANGE_COLS:
        ok = (on != 0) & (md[:, c] < 1 << 16)
        np.add.at(rng[:, 1], md[ok, c], on[ok])
    byte[:, rv32.Y_MULT] = 0
    cpu = np.asarray(tables[0], dtype=np.int64) % P
    bit_rows = cpu[cpu[:, rv32.IS_BIT] == 1]
    for k in range(4):
        key = (bit_rows[:, rv32.BOP] - 1) << 16 | bit_rows[:, rv32.BA + k] << 8 | bit_rows[:, rv32.BB + k]
        np.add.at(byte[:, rv32.Y_MULT], key, 1)
    for j, (u, v) in enumerate(rv32im.BYTE_PAIRS):
        ok = (on != 0) & (md[:, u] < 256) & (md[:, v] < 256) & (md[:, rv32im.D_AND + j] == (md[:, u] & md[:, v])) & \
            (md[:, rv32im.D_ONE] == 1)
        np.add.at(byte[:, rv32.Y_MULT], md[ok, u] << 8 | md[ok, v], on[ok])
    for j, col in enumerate(rv32im.SIGN_BYTES):
        x, lo, hi = md[:, col], md[:, rv32im.D_L + j], md[:, rv32im.D_S + j]
        ok = (on != 0) & (x < 256) & (lo == (2 * x) & 255) & (hi == x >> 7) & (md[:, rv32im.D_ONE] == 1)
        np.add.at(sh[:, rv32cf.H_MULT], 256 + x[ok], on[ok])
    rng[:, 1] %= P
    byte[:, rv32.Y_MULT] %= P
    sh[:, rv32cf.H_MULT] %= P
    return tables[:3] + [byte, rng, sh] + tables[6:]
