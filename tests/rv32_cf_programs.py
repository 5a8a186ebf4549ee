"""TEST INFRASTRUCTURE: the guest program and the hand-built traces of the rv32i-cf chip set tests: all six branches
taken and not taken at their signed / unsigned edges with forward and backward targets, JAL, JALR with an odd rs1 + imm,
the six shifts at the edge amounts (register amounts with bits above bit 4 set, SRA of negative values), a loop long
enough for several 2^13 shards; and a one-row shard helper for the traces an honest executor never writes."""
import numpy as np

import rv32_asm as A
from raiko_amd import rv32, rv32cf

HALT = A.li("t0", 0) + [("ecall",)]
AMOUNTS = (0, 1, 7, 8, 9, 15, 16, 24, 31)


def _branches():
    """every branch at 0x7FFFFFFF / 0x80000000, equal values, -1 / 0, taken and not taken; forward targets (skipping a
    poison `addi`) and one backward target per condition"""
    out = A.li("s0", 0x7FFFFFFF) + A.li("s1", 0x80000000) + A.li("s2", 0xFFFFFFFF) + [("addi", "s3", "zero", 0),
                                                                                         ("addi", "s4", "s0", 0)]
    pairs = [("s0", "s1"), ("s1", "s0"), ("s0", "s4"), ("s2", "s3"), ("s3", "s2")]
    n = 0
    for op in ("beq", "bne", "blt", "bge", "bltu", "bgeu"):
        for x, y in pairs:
            lab = "f%d" % n
            out += [(op, x, y, lab), ("addi", "a2", "a2", 1), lab + ":"]
            n += 1
        # backward: jump over the back block, the block comes back to a label before it only when the condition holds
        x, y = {"beq": ("s0", "s4"), "bne": ("s0", "s1"), "blt": ("s1", "s0"), "bge": ("s0", "s1"), "bltu": ("s0", "s1"),
                "bgeu": ("s1", "s0")}[op]
        out += [("jal", "zero", "fwd%d" % n), "back%d:" % n, ("jal", "zero", "done%d" % n), "fwd%d:" % n,
                (op, x, y, "back%d" % n), ("addi", "a2", "a2", 100), "done%d:" % n]
        n += 1
    return out


def _shifts():
    out = A.li("s5", 0x8765F0A1) + A.li("s6", 0x1234ABCD)
    for k in AMOUNTS:
        out += [("slli", "a3", "s5", k), ("srli", "a4", "s5", k), ("srai", "a5", "s5", k), ("srai", "a6", "s6", k)]
        # register amounts: k with bits above bit 4 set (0xFFFFFFE0 | k and 0x5A5A5A40 | k)
        out += A.li("s7", 0xFFFFFFE0 | k) + [("sll", "a3", "s5", "s7"), ("srl", "a4", "s5", "s7"), ("sra", "a5", "s5", "s7")]
        out += A.li("s7", 0x5A5A5A40 | k) + [("sra", "a6", "s6", "s7"), ("srl", "a7", "s2", "s7"), ("sll", "a7", "s2", "s7")]
    out += [("slli", "zero", "s5", 3)]                          # rd = x0: nothing written, the result is not bound
    return out


def _jumps():
    # JAL forward, JALR with an odd rs1 + imm (the low bit dropped: auipc + 1 + 16 -> j2) and with an even one
    return [("jal", "ra", "j1"), ("addi", "a2", "a2", 1000), "j1:", ("auipc", "t3", 0), ("addi", "t3", "t3", 1),
            ("jalr", "t4", 16, "t3"), ("addi", "a2", "a2", 1000), "j2:", ("auipc", "t3", 0), ("jalr", "t5", 12, "t3"),
            ("addi", "a2", "a2", 1000), "j3:", ("fence",)]


def cf_program(loops=1):
    """the control-flow and shift cases, `loops` passes of them (a backward bne closes the loop)"""
    body = _branches() + _shifts() + _jumps()
    prog = A.li("t0", 1) + A.li("a0", 0x300100) + [("addi", "a1", "zero", 4), ("ecall",)]
    prog += A.li("tp", loops) + ["loop:"] + body + [("addi", "tp", "tp", -1), ("bne", "tp", "zero", "loop")]
    prog += A.li("a0", 7) + HALT
    code, _ = A.assemble(prog)
    return A.elf(code, data=b"\0" * 0x200)


def one_row(chips, ins, a, b, nxt, res, pc=0x1000):
    """a one-cycle shard of `chips` ("rv32i" or "rv32i-cf") running instruction `ins` at `pc` on rs1 / rs2 values a / b
    and claiming next pc `nxt` and result `res` -- what an executor that takes any branch it likes, or shifts wrongly,
    would write.  Every other column is filled as that executor would fill it: under rv32i-cf TAKEN and the next pc's
    carries follow the claimed next pc, the decision's and the shift's own columns are the true ones (rv32cf.cpu_rows
    strict=False) -> canonical tables, cpu publics, register publics"""
    init = np.zeros(32, dtype=np.int64)
    init[(ins >> 15) & 31], init[(ins >> 20) & 31] = a, b
    tr = dict(pc=np.array([pc]), ins=np.array([ins]), a=np.array([a]), b=np.array([b]), res=np.array([res]),
              next=np.array([nxt]))
    ec = np.zeros((0, 2), dtype=np.int64)
    if chips == "rv32i":
        cpu, final, final_ts, hist, byte_mult = rv32.cpu_rows(tr, 2, nxt, init, ec)
        prog = rv32.program_table_for(tr["pc"], tr["ins"], pc, pc)
        extra = []
    else:
        cpu, final, final_ts, hist, byte_mult, shift_mult = rv32cf.cpu_rows(tr, 2, nxt, init, ec, strict=False)
        prog = rv32cf.program_table_for(tr["pc"], tr["ins"], pc, pc)
        extra = [rv32cf.shift_rows(shift_mult)]
    tables = [cpu, prog, rv32.register_rows(init, final, final_ts), rv32.byte_rows(byte_mult),
              np.stack([np.arange(1 << 16, dtype=np.int64), hist], axis=1)] + extra
    pub_cpu = np.array([pc & 0xFFFF, pc >> 16, nxt & 0xFFFF, nxt >> 16], dtype=np.int64)
    return tables, pub_cpu, rv32.register_publics(init, final)


# a taken BLT on a false condition (0x7FFFFFFF < 0x80000000 is false signed), and SLLI by 3 claiming a wrong result
BLT_FALSE = dict(ins=A.encode("blt", ("x1", "x2", 0x1040), 0x1000, {}), a=0x7FFFFFFF, b=0x80000000, nxt=0x1040, res=0)
SLLI_WRONG = dict(ins=A.encode("slli", ("x3", "x1", 3), 0x1000, {}), a=0x10000001, b=0, nxt=0x1004, res=0x80000009)


BRANCH_EDGES = [(0x7FFFFFFF, 0x80000000), (0x80000000, 0x7FFFFFFF), (5, 5), (0xFFFFFFFF, 0)]


def condition(op, a, b):
    sa, sb = a - (a >> 31 << 32), b - (b >> 31 << 32)
    return {"beq": a == b, "bne": a != b, "blt": sa < sb, "bge": sa >= sb, "bltu": a < b, "bgeu": a >= b}[op]


def branch_forgery(op, a, b, backward=False, pc=0x1000):
    """one_row arguments of branch `op` on rs1 / rs2 = a / b going the way its condition does not: to the target (pc -
    0x40 or pc + 0x40) when the condition is false, to pc + 4 when it holds"""
    target = pc - 0x40 if backward else pc + 0x40
    ins = A.encode(op, ("x1", "x2", target), pc, {})
    return dict(ins=ins, a=a, b=b, nxt=pc + 4 if condition(op, a, b) else target, res=0, pc=pc)


def balance(tables):
    """an rv32i-cf shard's range and shift counts recomputed from what its cpu table sends, as a forger who edited cpu
    cells would: only values those tables hold can be counted"""
    from raiko_amd.segment import P
    cpu = np.asarray(tables[0], dtype=np.int64) % P
    rng, sh = tables[4].copy(), tables[5].copy()
    rng[:, 1] = 0
    for c, m in rv32cf.RANGE_SENDS:
        ok = (cpu[:, m] != 0) & (cpu[:, c] < 1 << 16)
        np.add.at(rng[:, 1], cpu[ok, c], cpu[ok, m])
    sh[:, rv32cf.H_MULT] = 0
    for j in range(4):
        k, x, lo, hi = cpu[:, rv32cf.SK], cpu[:, rv32cf.SX + j], cpu[:, rv32cf.SLO + j], cpu[:, rv32cf.SHI + j]
        ok = (cpu[:, rv32cf.IS_SHIFT] != 0) & (k <= 8) & (x < 256)
        v = np.where(ok, x, 0) << np.where(ok, k, 0)
        ok &= (lo == v & 255) & (hi == v >> 8)
        np.add.at(sh[:, rv32cf.H_MULT], (k * 256 + x)[ok], cpu[ok, rv32cf.IS_SHIFT])
    rng[:, 1] %= P
    sh[:, rv32cf.H_MULT] %= P
    return list(tables[:4]) + [rng, sh] + list(tables[6:])


def set_shift(cpu, r, kb, q, t):
    """row r's shift columns rewritten for the amount bits kb (three values, a bit each when honest), the one-hot index q
    and the quotient t, with the shifted bytes, their table parts and the assembled result that amount gives"""
    M = 0xFFFFFFFF
    k = kb[0] + 2 * kb[1] + 4 * kb[2]
    s = k + 8 * q
    left = cpu[r, rv32cf.IS_SLL] == 1
    a = int(cpu[r, rv32.A_LO] | cpu[r, rv32.A_HI] << 16)
    fill = int(cpu[r, rv32cf.FILL])
    ap = a ^ (M * fill)
    sk = k if left else 8 - k
    u = ((ap << s) & M) if left else ap >> s
    cpu[r, rv32cf.KB:rv32cf.KB + 3] = kb
    cpu[r, rv32cf.Q:rv32cf.Q + 4] = 0
    cpu[r, rv32cf.Q + q] = 1
    cpu[r, rv32cf.T], cpu[r, rv32cf.SK] = t, sk
    for j in range(4):
        x = (ap >> (8 * j)) & 255
        cpu[r, rv32cf.SX + j], cpu[r, rv32cf.SLO + j], cpu[r, rv32cf.SHI + j] = x, (x << sk) & 255, (x << sk) >> 8
    v = u ^ (M * fill)
    cpu[r, rv32cf.U_LO], cpu[r, rv32cf.U_HI], cpu[r, rv32cf.V_LO], cpu[r, rv32cf.V_HI] = u & 0xFFFF, u >> 16, v & 0xFFFF, v >> 16
    return v
