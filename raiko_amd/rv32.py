"""The rv32i chip set: an executed segment proven as a uni-stark shard whose AIRs constrain the register file and the
integer ALU, not only the pc chain (p3_trace.p3_trace_air).  Five tables per shard, tied by lookups:

  cpu       one row per cycle (RV32_CPU_COLS columns): the stand-in trace's 16 columns at their old places, the decoded
            fields the row looks up in the program table, three register accesses with their previous timestamps, the
            ALU's operand / carry / borrow / sign / byte columns
  program   one row per word of the executed pc range: (pc, instruction) and the fields decoded from the word's 32 bits,
            which the program AIR proves from those bits; receives PROGRAM tuples
  register  32 rows: sends every register's initial value at timestamp 0, receives its final (value, timestamp); both are
            bound to the shard's public values through shift registers of 32 columns per limb stream
  byte      2^18 rows (3 * 2^16 used): (op, x, y, x op y) for AND / OR / XOR of two bytes, proven from their bits
  range     p3_trace.p3_range_air: the 16-bit values

Registers follow an offline memory argument on the REGISTER bus: access k of row r (k = 1 read rs1, 2 read rs2, 3 write
the destination) happens at timestamp 3r + k, receives (reg, previous value, previous timestamp) and sends (reg, value,
timestamp); ts - prev_ts - 1 = lo + 2^14 hi with lo, hi looked up in RANGE16, so 0 <= ts - prev_ts - 1 < 2^30 < p.

Constrained: the value written to rd by ADD, SUB, ADDI, AND, OR, XOR, ANDI, ORI, XORI, SLT, SLTU, SLTI, SLTIU, LUI,
AUIPC and the link value pc + 4 of JAL / JALR.  Free (witness cells the AIR does not tie to anything): results of
shifts, the M extension and loads; branch / jump decisions and targets (a `seq` row keeps the pc + 4 constraint);
memory (a store is two register reads); the a0 an ecall leaves (every ecall row writes x10 with a free value).
rv32cf.py builds the rv32i-cf chip set on this one (the same cpu / program bodies and columns, more appended): there
branches, jumps, the next pc of every row and the shifts are constrained too.
The witness recomputes the ALU result of constrained ops (TraceRow.res is 0 when rd is x0), so the ALU constraints
hold on every active row, written or not.

`shard_tables` builds every table of a segment in numpy from the recorded trace and the executor's side data
(rv32_sets.p3_rv32_shards): the yardstick for rk_exec_rv32_shard_device."""
import numpy as np

from .p3_trace import p3_range_air
from .segment import P

BUS_PROGRAM, BUS_RANGE16, BUS_REGISTER, BUS_BYTE = 1, 2, 5, 6
N_PUBLIC_CPU = 4           # start pc lo / hi, end pc lo / hi
N_PUBLIC_REG = 128         # initial x0..x31 lo / hi, then final x0..x31 lo / hi

# ---- cpu columns (the first 16 are the stand-in trace's, at the same places)
PC_LO, PC_HI, NX_LO, NX_HI, INS_LO, INS_HI, SEQ, CARRY, A_LO, A_HI, B_LO, B_HI, RES_LO, RES_HI, WR, ACTIVE = range(16)
(RS1, RS2, WREG, IMM_LO, IMM_HI, IS_ADD, IS_SUB, IS_SLT, IS_SLTU, IS_BIT, BOP, IS_IMM, IS_LUI, IS_AUIPC, IS_LINK,
 TSA, TSB, TSW, PA_TS, PB_TS, PW_TS, PW_LO, PW_HI, DA_LO, DA_HI, DB_LO, DB_HI, DW_LO, DW_HI,
 OB_LO, OB_HI, C0, C1, D_LO, D_HI, SA, SB, SNE, SA_CHK, SB_CHK) = range(16, 56)
BA, BB, BR = 56, 60, 64        # bytes of rs1's value, of operand b, of the result (4 each)
CPU_COLS = 68
# what a cpu row looks up in the program table, in the order of the program table's first columns
PROGRAM_TUPLE = [PC_LO, PC_HI, INS_LO, INS_HI, RS1, RS2, WREG, IMM_LO, IMM_HI, IS_ADD, IS_SUB, IS_SLT, IS_SLTU, IS_BIT,
                 BOP, IS_IMM, IS_LUI, IS_AUIPC, IS_LINK, WR]

# ---- program columns: 0..19 the tuple above, then
P_MULT, P_BITS, P_OPC, P_F3, P_OPR, P_Z1, P_Z2, P_RDZ, P_RD = 20, 21, 53, 64, 72, 73, 74, 75, 76
PROGRAM_COLS = 77
OPCODES = (0x37, 0x17, 0x6F, 0x67, 0x63, 0x03, 0x23, 0x13, 0x33, 0x0F, 0x73)   # the selectors P_OPC + k, in this order
O_LUI, O_AUIPC, O_JAL, O_JALR, O_BRANCH, O_LOAD, O_STORE, O_OPIMM, O_OP, O_FENCE, O_SYSTEM = range(11)

# ---- register table columns
R_REG, R_ZERO, R_FTS, R_IL, R_IH, R_FL, R_FH = 0, 1, 2, 3, 35, 67, 99
REG_COLS = 131

# ---- byte table columns; ops AND = 1, OR = 2, XOR = 3
Y_OP, Y_X, Y_Y, Y_Z, Y_XB, Y_YB, Y_AND, Y_OR, Y_XOR, Y_MULT = 0, 1, 2, 3, 4, 12, 20, 21, 22, 23
BYTE_COLS, BYTE_LOG_ROWS = 24, 18

RANGE_SENDS = [(c, ACTIVE) for c in (PC_LO, PC_HI, NX_LO, NX_HI, RES_LO, RES_HI, D_LO, D_HI, DA_LO, DA_HI, DB_LO, DB_HI)] + \
    [(DW_LO, WR), (DW_HI, WR), (SA_CHK, IS_SLT), (SB_CHK, IS_SLT)]


def cpu_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(CPU_COLS, N_PUBLIC_CPU, p3.EXT_W if ext_w is None else ext_w)
    cpu_constraints(b, PROGRAM_TUPLE)
    return b.build()


def cpu_constraints(b, program_tuple):
    """the rv32i cpu AIR's interactions and constraints into builder b (whose width may be wider: the rv32i-cf cpu
    table appends its columns, rv32cf.py); program_tuple: the cpu columns looked up in the program table"""
    L = b.local
    b.send(BUS_PROGRAM, program_tuple, mult=ACTIVE, mult_is_const=False)
    b.receive(BUS_REGISTER, [RS1, A_LO, A_HI, PA_TS], mult=ACTIVE, mult_is_const=False)
    b.send(BUS_REGISTER, [RS1, A_LO, A_HI, TSA], mult=ACTIVE, mult_is_const=False)
    b.receive(BUS_REGISTER, [RS2, B_LO, B_HI, PB_TS], mult=ACTIVE, mult_is_const=False)
    b.send(BUS_REGISTER, [RS2, B_LO, B_HI, TSB], mult=ACTIVE, mult_is_const=False)
    b.receive(BUS_REGISTER, [WREG, PW_LO, PW_HI, PW_TS], mult=WR, mult_is_const=False)
    b.send(BUS_REGISTER, [WREG, RES_LO, RES_HI, TSW], mult=WR, mult_is_const=False)
    for k in range(4):
        b.send(BUS_BYTE, [BOP, BA + k, BB + k, BR + k], mult=IS_BIT, mult_is_const=False)
    for c, m in RANGE_SENDS:
        b.send(BUS_RANGE16, [c], mult=m, mult_is_const=False)
    # the pc chain of the stand-in trace AIR
    pc_lo, pc_hi, nx_lo, nx_hi = (L(c) for c in range(4))
    seq, carry, wr, active = L(SEQ), L(CARRY), L(WR), L(ACTIVE)
    for v in (seq, carry, wr, active, L(C0), L(C1), L(SA), L(SB)):
        b.assert_zero(v * (v - 1))
    b.assert_zero(seq * (nx_lo - pc_lo - 4 + carry * 65536))
    b.assert_zero(seq * (nx_hi - pc_hi - carry))
    t = b.when_transition()
    t.assert_eq(b.next(PC_LO), nx_lo)
    t.assert_eq(b.next(PC_HI), nx_hi)
    t.assert_zero((1 - active) * b.next(ACTIVE))
    b.assert_zero((1 - active) * seq)
    # every multiplicity that is a column is 0 on padding rows: ACTIVE itself, WR and the two the program lookup binds
    # only on active rows (a padding row with IS_BIT or IS_SLT = -1 would receive what an active row sends)
    b.assert_zero((1 - active) * wr)
    b.assert_zero((1 - active) * L(IS_BIT))
    b.assert_zero((1 - active) * L(IS_SLT))
    f = b.when_first_row()
    f.assert_eq(pc_lo, b.public(0))
    f.assert_eq(pc_hi, b.public(1))
    last = b.when_last_row()
    last.assert_eq(nx_lo, b.public(2))
    last.assert_eq(nx_hi, b.public(3))
    # timestamps: 3 row + 1 / 2 / 3, and every access after the one it follows
    f.assert_eq(L(TSA), 1)
    t.assert_eq(b.next(TSA), L(TSA) + 3)
    b.assert_eq(L(TSB), L(TSA) + 1)
    b.assert_eq(L(TSW), L(TSA) + 2)
    b.assert_zero(active * (L(TSA) - L(PA_TS) - 1 - L(DA_LO) - L(DA_HI) * 16384))
    b.assert_zero(active * (L(TSB) - L(PB_TS) - 1 - L(DB_LO) - L(DB_HI) * 16384))
    b.assert_zero(wr * (L(TSW) - L(PW_TS) - 1 - L(DW_LO) - L(DW_HI) * 16384))
    # operand b: rs2's value or the immediate
    imm = L(IS_IMM)
    b.assert_eq(L(OB_LO), L(B_LO) + imm * (L(IMM_LO) - L(B_LO)))
    b.assert_eq(L(OB_HI), L(B_HI) + imm * (L(IMM_HI) - L(B_HI)))
    a_lo, a_hi, ob_lo, ob_hi, r_lo, r_hi = L(A_LO), L(A_HI), L(OB_LO), L(OB_HI), L(RES_LO), L(RES_HI)
    c0, c1, d_lo, d_hi = L(C0), L(C1), L(D_LO), L(D_HI)
    add = L(IS_ADD)
    b.assert_zero(add * (a_lo + ob_lo - r_lo - c0 * 65536))
    b.assert_zero(add * (a_hi + ob_hi + c0 - r_hi - c1 * 65536))
    sub, slt, sltu = L(IS_SUB), L(IS_SLT), L(IS_SLTU)
    sublt = sub + slt + sltu                     # a = d + operand b (mod 2^32); c1 = borrow of a - operand b
    b.assert_zero(sublt * (d_lo + ob_lo - a_lo - c0 * 65536))
    b.assert_zero(sublt * (d_hi + ob_hi + c0 - a_hi - c1 * 65536))
    b.assert_zero(sub * (r_lo - d_lo))
    b.assert_zero(sub * (r_hi - d_hi))
    b.assert_zero(sltu * (r_lo - c1))
    b.assert_zero(sltu * r_hi)
    sa, sb, sne = L(SA), L(SB), L(SNE)
    b.assert_eq(sne, sa + sb - sa * sb * 2)
    b.assert_eq(L(SA_CHK), a_hi * 2 - sa * 65536)     # SA_CHK < 2^16 (RANGE16 on SLT rows): sa is a_hi's top bit
    b.assert_eq(L(SB_CHK), ob_hi * 2 - sb * 65536)
    b.assert_zero(slt * (r_lo - sa * (1 - sb) - (1 - sne) * c1))
    b.assert_zero(slt * r_hi)
    lui, auipc, link = L(IS_LUI), L(IS_AUIPC), L(IS_LINK)
    b.assert_zero(lui * (r_lo - L(IMM_LO)))
    b.assert_zero(lui * (r_hi - L(IMM_HI)))
    b.assert_zero(auipc * (pc_lo + L(IMM_LO) - r_lo - c0 * 65536))
    b.assert_zero(auipc * (pc_hi + L(IMM_HI) + c0 - r_hi - c1 * 65536))
    b.assert_zero(link * (pc_lo + 4 - r_lo - c0 * 65536))
    b.assert_zero(link * (pc_hi + c0 - r_hi - c1 * 65536))
    bit = L(IS_BIT)
    for base, lo, hi in ((BA, a_lo, a_hi), (BB, ob_lo, ob_hi), (BR, r_lo, r_hi)):
        b.assert_zero(bit * (lo - L(base) - L(base + 1) * 256))
        b.assert_zero(bit * (hi - L(base + 2) - L(base + 3) * 256))


def program_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(PROGRAM_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    program_constraints(b, list(range(20)))
    return b.build()


def lin(terms):
    """sum of expression * constant over (expression, constant) pairs"""
    acc = None
    for e, c in terms:
        x = e * c if c != 1 else e
        acc = x if acc is None else acc + x
    return acc


def program_constraints(b, tuple_cols):
    """the rv32i program AIR's interaction and constraints into builder b (the rv32i-cf program table appends its
    columns, rv32cf.py); tuple_cols: the program columns the PROGRAM bus receives"""
    L = b.local
    b.receive(BUS_PROGRAM, tuple_cols, mult=P_MULT, mult_is_const=False)
    bit = [L(P_BITS + i) for i in range(32)]
    opc = [L(P_OPC + k) for k in range(11)]
    f3 = [L(P_F3 + j) for j in range(8)]
    for v in bit + opc + f3:
        b.assert_zero(v * (v - 1))
    b.assert_eq(L(2), lin([(bit[i], 1 << i) for i in range(16)]))
    b.assert_eq(L(3), lin([(bit[16 + i], 1 << i) for i in range(16)]))
    s = lin([(o, 1) for o in opc])
    b.assert_zero(s * (s - 1))                   # at most one opcode class ...
    b.assert_zero(L(P_MULT) * (1 - s))           # ... and exactly one on a row a cpu row may look up
    b.assert_eq(lin([(o, v) for o, v in zip(opc, OPCODES)]), lin([(bit[i], 1 << i) for i in range(7)]))
    b.assert_eq(lin([(x, 1) for x in f3]), s)
    b.assert_eq(lin([(f3[j], j) for j in range(1, 8)]), lin([(bit[12], 1), (bit[13], 2), (bit[14], 4)]))
    b.assert_eq(L(P_RD), lin([(bit[7 + i], 1 << i) for i in range(5)]))
    b.assert_eq(L(4), lin([(bit[15 + i], 1 << i) for i in range(5)]))
    b.assert_eq(L(5), lin([(bit[20 + i], 1 << i) for i in range(5)]))
    b.assert_eq(L(P_Z1), (1 - bit[7]) * (1 - bit[8]))
    b.assert_eq(L(P_Z2), L(P_Z1) * (1 - bit[9]))
    b.assert_eq(L(P_RDZ), L(P_Z2) * (1 - bit[10]) * (1 - bit[11]))
    b.assert_eq(L(P_OPR), opc[O_OP] * (1 - bit[25]))      # OP without the M extension
    opr, opimm = L(P_OPR), opc[O_OPIMM]
    alu = opr + opimm
    b.assert_eq(L(9), opr * f3[0] * (1 - bit[30]) + opimm * f3[0])
    b.assert_eq(L(10), opr * f3[0] * bit[30])
    b.assert_eq(L(11), alu * f3[2])
    b.assert_eq(L(12), alu * f3[3])
    b.assert_eq(L(13), alu * (f3[4] + f3[6] + f3[7]))
    b.assert_eq(L(14), alu * (f3[4] * 3 + f3[6] * 2 + f3[7]))
    b.assert_eq(L(15), opimm)
    b.assert_eq(L(16), opc[O_LUI])
    b.assert_eq(L(17), opc[O_AUIPC])
    b.assert_eq(L(18), opc[O_JAL] + opc[O_JALR])
    writes = lin([(opc[k], 1) for k in (O_LUI, O_AUIPC, O_JAL, O_JALR, O_LOAD, O_OPIMM, O_OP)])
    b.assert_eq(L(19), writes * (1 - L(P_RDZ)) + opc[O_SYSTEM])
    b.assert_eq(L(6), L(P_RD) + opc[O_SYSTEM] * 10)
    sel_i = opimm + opc[O_LOAD] + opc[O_JALR]
    sel_u = opc[O_LUI] + opc[O_AUIPC]
    i_lo = lin([(bit[20 + i], 1 << i) for i in range(11)] + [(bit[31], 65536 - 2048)])
    u_lo = lin([(bit[i], 1 << i) for i in range(12, 16)])
    b.assert_eq(L(7), sel_i * i_lo + sel_u * u_lo)
    b.assert_eq(L(8), sel_i * (bit[31] * 65535) + sel_u * L(3))


def register_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(REG_COLS, N_PUBLIC_REG, p3.EXT_W if ext_w is None else ext_w)
    L = b.local
    b.send(BUS_REGISTER, [R_REG, R_IL, R_IH, R_ZERO])
    b.receive(BUS_REGISTER, [R_REG, R_FL, R_FH, R_FTS])
    f, t = b.when_first_row(), b.when_transition()
    f.assert_zero(L(R_REG))
    t.assert_eq(b.next(R_REG), L(R_REG) + 1)
    b.assert_zero(L(R_ZERO))
    f.assert_zero(L(R_IL))                       # x0 starts at 0 (and no row writes it)
    f.assert_zero(L(R_IH))
    for s, off in ((R_IL, 0), (R_IH, 1), (R_FL, 64), (R_FH, 65)):
        for j in range(32):
            f.assert_eq(L(s + j), b.public(off + 2 * j))
            if j < 31:
                t.assert_eq(b.next(s + j), L(s + j + 1))
    return b.build()


def byte_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(BYTE_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    L = b.local
    b.receive(BUS_BYTE, [Y_OP, Y_X, Y_Y, Y_Z], mult=Y_MULT, mult_is_const=False)
    xb = [L(Y_XB + i) for i in range(8)]
    yb = [L(Y_YB + i) for i in range(8)]
    s_and, s_or, s_xor = L(Y_AND), L(Y_OR), L(Y_XOR)
    for v in xb + yb + [s_and, s_or, s_xor]:
        b.assert_zero(v * (v - 1))
    s = s_and + s_or + s_xor
    b.assert_zero(s * (s - 1))
    b.assert_eq(L(Y_OP), s_and + s_or * 2 + s_xor * 3)

    def sum8(terms):
        acc = terms[0]
        for i in range(1, 8):
            acc = acc + terms[i] * (1 << i)
        return acc

    b.assert_eq(L(Y_X), sum8(xb))
    b.assert_eq(L(Y_Y), sum8(yb))
    xy = [x * y for x, y in zip(xb, yb)]
    z = L(Y_Z)
    b.assert_zero(s_and * (z - sum8(xy)))
    b.assert_zero(s_or * (z - sum8([x + y - p for x, y, p in zip(xb, yb, xy)])))
    b.assert_zero(s_xor * (z - sum8([x + y - p * 2 for x, y, p in zip(xb, yb, xy)])))
    return b.build()


def airs(ext_w=None):
    """-> (cpu, program, register, byte, range): the AIRs of one rv32i shard, in table order"""
    return cpu_air(ext_w), program_air(ext_w), register_air(ext_w), byte_air(ext_w), p3_range_air(ext_w)


# ------------------------------------------------------------------------------------------------ numpy witness
def _u(x):
    return np.asarray(x, dtype=np.int64)


def decode(ins):
    """decoded program-table fields of instruction words (int64 array) -> dict of int64 arrays (PROGRAM_TUPLE order
    for indices 4..19 plus the helper columns)"""
    ins = _u(ins) & 0xFFFFFFFF
    bits = (ins[:, None] >> np.arange(32)) & 1
    op7 = ins & 0x7F
    opc = np.stack([(op7 == v) for v in OPCODES], axis=1).astype(np.int64)
    valid = opc.sum(axis=1)
    f3v = (ins >> 12) & 7
    f3 = np.stack([(f3v == j) for j in range(8)], axis=1).astype(np.int64) * valid[:, None]
    rd, rs1, rs2 = (ins >> 7) & 31, (ins >> 15) & 31, (ins >> 20) & 31
    z1 = (1 - bits[:, 7]) * (1 - bits[:, 8])
    z2 = z1 * (1 - bits[:, 9])
    rdz = z2 * (1 - bits[:, 10]) * (1 - bits[:, 11])
    opr = opc[:, O_OP] * (1 - bits[:, 25])
    opimm = opc[:, O_OPIMM]
    alu = opr + opimm
    sel_i = opimm + opc[:, O_LOAD] + opc[:, O_JALR]
    sel_u = opc[:, O_LUI] + opc[:, O_AUIPC]
    i_imm = np.where(bits[:, 31] == 1, (ins >> 20) | 0xFFFFF000, ins >> 20) & 0xFFFFFFFF
    u_imm = ins & 0xFFFFF000
    imm = sel_i * i_imm + sel_u * u_imm
    writes = opc[:, [O_LUI, O_AUIPC, O_JAL, O_JALR, O_LOAD, O_OPIMM, O_OP]].sum(axis=1)
    d = dict(rs1=rs1, rs2=rs2, wreg=rd + 10 * opc[:, O_SYSTEM], imm_lo=imm & 0xFFFF, imm_hi=imm >> 16,
             is_add=opr * f3[:, 0] * (1 - bits[:, 30]) + opimm * f3[:, 0], is_sub=opr * f3[:, 0] * bits[:, 30],
             is_slt=alu * f3[:, 2], is_sltu=alu * f3[:, 3], is_bit=alu * (f3[:, 4] + f3[:, 6] + f3[:, 7]),
             bop=alu * (3 * f3[:, 4] + 2 * f3[:, 6] + f3[:, 7]), is_imm=opimm, is_lui=opc[:, O_LUI],
             is_auipc=opc[:, O_AUIPC], is_link=opc[:, O_JAL] + opc[:, O_JALR], wr=writes * (1 - rdz) + opc[:, O_SYSTEM],
             bits=bits, opc=opc, f3=f3, opr=opr, z1=z1, z2=z2, rdz=rdz, rd=rd, imm=imm)
    return d


_DECODED = ["rs1", "rs2", "wreg", "imm_lo", "imm_hi", "is_add", "is_sub", "is_slt", "is_sltu", "is_bit", "bop", "is_imm",
            "is_lui", "is_auipc", "is_link", "wr"]


def program_rows(pcs, inss, counts, n_rows):
    """program table (canonical int64): row s = (pc, instruction, decoded fields, multiplicity, bits, selectors...);
    rows past the given ones are the row of word 0 at pc 0 with multiplicity 0"""
    t = np.zeros((n_rows, PROGRAM_COLS), dtype=np.int64)
    k = len(pcs)
    pcs_all, ins_all = np.zeros(n_rows, dtype=np.int64), np.zeros(n_rows, dtype=np.int64)
    pcs_all[:k], ins_all[:k] = pcs, inss
    d = decode(ins_all)
    t[:, 0], t[:, 1] = pcs_all & 0xFFFF, pcs_all >> 16
    t[:, 2], t[:, 3] = ins_all & 0xFFFF, ins_all >> 16
    for j, name in enumerate(_DECODED):
        t[:, 4 + j] = d[name]
    t[:k, P_MULT] = counts
    t[:, P_BITS:P_BITS + 32] = d["bits"]
    t[:, P_OPC:P_OPC + 11] = d["opc"]
    t[:, P_F3:P_F3 + 8] = d["f3"]
    t[:, P_OPR], t[:, P_Z1], t[:, P_Z2], t[:, P_RDZ], t[:, P_RD] = d["opr"], d["z1"], d["z2"], d["rdz"], d["rd"]
    return t


def byte_rows(mult=None):
    n = 1 << BYTE_LOG_ROWS
    r = np.arange(3 << 16, dtype=np.int64)
    op, x, y = (r >> 16) + 1, (r >> 8) & 255, r & 255
    z = np.where(op == 1, x & y, np.where(op == 2, x | y, x ^ y))
    t = np.zeros((n, BYTE_COLS), dtype=np.int64)
    t[: r.size, Y_OP], t[: r.size, Y_X], t[: r.size, Y_Y], t[: r.size, Y_Z] = op, x, y, z
    t[: r.size, Y_XB:Y_XB + 8] = (x[:, None] >> np.arange(8)) & 1
    t[: r.size, Y_YB:Y_YB + 8] = (y[:, None] >> np.arange(8)) & 1
    for k, c in enumerate((Y_AND, Y_OR, Y_XOR)):
        t[: r.size, c] = op == k + 1
    if mult is not None:
        t[: r.size, Y_MULT] = mult[: r.size]
    return t


def register_rows(init, final, final_ts):
    t = np.zeros((32, REG_COLS), dtype=np.int64)
    t[:, R_REG] = np.arange(32)
    t[:, R_FTS] = final_ts
    for s, vals in ((R_IL, _u(init) & 0xFFFF), (R_IH, _u(init) >> 16), (R_FL, _u(final) & 0xFFFF), (R_FH, _u(final) >> 16)):
        for j in range(32):
            t[: 32 - j, s + j] = vals[j:]
    return t


def register_publics(init, final):
    init, final = _u(init), _u(final)
    return np.concatenate([np.stack([init & 0xFFFF, init >> 16], axis=1).reshape(-1),
                           np.stack([final & 0xFFFF, final >> 16], axis=1).reshape(-1)])


def cpu_rows(tr, n, end_pc, init, ecalls):
    """tr: dict of int64 arrays over the executed cycles (pc, ins, a, b, res, next); init: the 32 registers at the
    segment's start; ecalls: (cycle, a0 after) of every ecall row -> (cpu table (n, CPU_COLS) int64, final values,
    final timestamps, RANGE16 histogram, BYTE multiplicities)"""
    cyc = tr["pc"].size
    t = np.zeros((n, CPU_COLS), dtype=np.int64)
    pc, ins, a, bv, nxt = (_u(tr[k]) for k in ("pc", "ins", "a", "b", "next"))
    d = decode(ins)
    imm = d["imm"]
    ob = np.where(d["is_imm"] == 1, imm, bv)
    res = _u(tr["res"]).copy()
    M = 0xFFFFFFFF
    sa, sb = a >> 31, ob >> 31
    lt_u = (a < ob).astype(np.int64)
    lt_s = np.where(sa != sb, sa, lt_u)
    f3v = (ins >> 12) & 7
    bitw = np.where(f3v == 4, a ^ ob, np.where(f3v == 6, a | ob, a & ob))
    for sel, val in (("is_add", (a + ob) & M), ("is_sub", (a - ob) & M), ("is_slt", lt_s), ("is_sltu", lt_u),
                     ("is_bit", bitw), ("is_lui", imm), ("is_auipc", (pc + imm) & M), ("is_link", (pc + 4) & M)):
        res = np.where(d[sel] == 1, val, res)
    sysrow = (ins & 0x7F) == 0x73
    ec = np.asarray(ecalls, dtype=np.int64).reshape(-1, 2)
    if sysrow.any():
        want = np.nonzero(sysrow)[0]
        if ec.shape[0] != want.size or not np.array_equal(ec[:, 0], want):
            raise ValueError("ecall side list does not match the trace")
        res[want] = ec[:, 1]
    wr = d["wr"]
    # carries: ADD / AUIPC / link: x + y = res + c 2^32; SUB / SLT*: operand b + d = a + c 2^32
    x = np.where(d["is_add"] == 1, a, np.where(d["is_auipc"] + d["is_link"] > 0, pc, 0))
    y = np.where(d["is_add"] == 1, ob, np.where(d["is_auipc"] == 1, imm, np.where(d["is_link"] == 1, 4, 0)))
    sublt = d["is_sub"] + d["is_slt"] + d["is_sltu"]
    dd = np.where(sublt == 1, (a - ob) & M, 0)
    x = np.where(sublt == 1, dd, x)
    y = np.where(sublt == 1, ob, y)
    c0 = ((x & 0xFFFF) + (y & 0xFFFF)) >> 16
    c1 = ((x >> 16) + (y >> 16) + c0) >> 16
    # register accesses, in timestamp order per register
    rows = np.arange(cyc, dtype=np.int64)
    tsa = 3 * rows + 1
    regs = np.concatenate([d["rs1"], d["rs2"], np.where(wr == 1, d["wreg"], -1)])
    ts = np.concatenate([tsa, tsa + 1, tsa + 2])
    val = np.concatenate([a, bv, res])
    keep = regs >= 0
    regs_k, ts_k, val_k = regs[keep], ts[keep], val[keep]
    order = np.lexsort((ts_k, regs_k))
    rs, tss, vs = regs_k[order], ts_k[order], val_k[order]
    first = np.ones(rs.size, dtype=bool)
    first[1:] = rs[1:] != rs[:-1]
    prev_ts = np.where(first, 0, np.roll(tss, 1))
    prev_val = np.where(first, _u(init)[rs] if rs.size else 0, np.roll(vs, 1))
    pts = np.zeros(ts.size, dtype=np.int64)
    pval = np.zeros(ts.size, dtype=np.int64)
    idx = np.nonzero(keep)[0][order]
    pts[idx], pval[idx] = prev_ts, prev_val
    final = _u(init).copy()
    final_ts = np.zeros(32, dtype=np.int64)
    last = np.ones(rs.size, dtype=bool)
    last[:-1] = rs[:-1] != rs[1:]
    final[rs[last]], final_ts[rs[last]] = vs[last], tss[last]
    pa_ts, pb_ts, pw_ts = pts[:cyc], pts[cyc:2 * cyc], pts[2 * cyc:]
    pw = pval[2 * cyc:]
    if not (np.array_equal(pval[:cyc], a) and np.array_equal(pval[cyc:2 * cyc], bv)):
        raise ValueError("a register read does not see the value last written")
    # the columns
    act = slice(0, cyc)
    lo = lambda v: v & 0xFFFF
    hi = lambda v: v >> 16
    carry = (((pc & 0xFFFF) + 4) > 0xFFFF).astype(np.int64)
    seq = ((nxt == pc + 4) & (pc <= 0xFFFFFFFB)).astype(np.int64)
    cols = {PC_LO: lo(pc), PC_HI: hi(pc), NX_LO: lo(nxt), NX_HI: hi(nxt), INS_LO: lo(ins), INS_HI: hi(ins), SEQ: seq,
            CARRY: seq * carry, A_LO: lo(a), A_HI: hi(a), B_LO: lo(bv), B_HI: hi(bv), RES_LO: lo(res), RES_HI: hi(res),
            WR: wr, ACTIVE: 1, RS1: d["rs1"], RS2: d["rs2"], WREG: d["wreg"], IMM_LO: d["imm_lo"], IMM_HI: d["imm_hi"],
            IS_ADD: d["is_add"], IS_SUB: d["is_sub"], IS_SLT: d["is_slt"], IS_SLTU: d["is_sltu"], IS_BIT: d["is_bit"],
            BOP: d["bop"], IS_IMM: d["is_imm"], IS_LUI: d["is_lui"], IS_AUIPC: d["is_auipc"], IS_LINK: d["is_link"],
            PA_TS: pa_ts, PB_TS: pb_ts, PW_TS: wr * pw_ts, PW_LO: wr * lo(pw), PW_HI: wr * hi(pw),
            OB_LO: lo(ob), OB_HI: hi(ob), C0: c0, C1: c1, D_LO: lo(dd), D_HI: hi(dd), SA: sa, SB: sb,
            SNE: sa ^ sb, SA_CHK: 2 * hi(a) - 65536 * sa, SB_CHK: 2 * hi(ob) - 65536 * sb}
    da, db, dw = tsa - pa_ts - 1, tsa + 1 - pb_ts - 1, wr * (tsa + 2 - pw_ts - 1)
    for c, v in ((DA_LO, da & 0x3FFF), (DA_HI, da >> 14), (DB_LO, db & 0x3FFF), (DB_HI, db >> 14),
                 (DW_LO, dw & 0x3FFF), (DW_HI, dw >> 14)):
        cols[c] = v
    for base, v in ((BA, a), (BB, ob), (BR, res)):
        for k in range(4):
            cols[base + k] = d["is_bit"] * ((v >> (8 * k)) & 255)
    for c, v in cols.items():
        t[act, c] = v
    t[cyc:, PC_LO], t[cyc:, PC_HI], t[cyc:, NX_LO], t[cyc:, NX_HI] = end_pc & 0xFFFF, end_pc >> 16, end_pc & 0xFFFF, end_pc >> 16
    allrows = np.arange(n, dtype=np.int64)
    t[:, TSA], t[:, TSB], t[:, TSW] = 3 * allrows + 1, 3 * allrows + 2, 3 * allrows + 3
    # multiplicities
    hist = np.zeros(1 << 16, dtype=np.int64)
    for c, m in RANGE_SENDS:
        sel = t[:, m] != 0
        hist += np.bincount(t[sel, c], minlength=1 << 16)[: 1 << 16]
    byte_mult = np.zeros(3 << 16, dtype=np.int64)
    bit_rows = t[t[:, IS_BIT] == 1]
    for k in range(4):
        key = (bit_rows[:, BOP] - 1) << 16 | bit_rows[:, BA + k] << 8 | bit_rows[:, BB + k]
        byte_mult += np.bincount(key, minlength=3 << 16)
    return t, final, final_ts, hist, byte_mult


def program_table_for(pcs, inss, pc_lo, pc_hi):
    """one row per word of [pc_lo, pc_hi] (rows padded to a power of two >= 2): the words executed in the shard with
    how often, the rest with instruction 0 and multiplicity 0"""
    slots = (pc_hi - pc_lo) // 4 + 1 if pcs.size else 0
    n_rows = 2
    while n_rows < slots:
        n_rows <<= 1
    s = (pcs - pc_lo) // 4
    cnt = np.bincount(s, minlength=slots).astype(np.int64)
    word = np.zeros(slots, dtype=np.int64)
    word[s] = inss
    if pcs.size and not np.array_equal(word[s], inss):
        raise ValueError("a pc executed with two different instruction words in one shard")
    slot_pc = pc_lo + 4 * np.arange(slots, dtype=np.int64)
    return program_rows(slot_pc, word, cnt, n_rows)


def trace_of(seg, data):
    """the 16 data columns of a segment's stand-in trace (Montgomery, (16, n)) -> (tr: dict of int64 arrays over the
    executed cycles (pc, next, ins, a, b, res, wr), n, the lowest and the highest pc executed: 0, 0 without cycles)"""
    from . import p3
    vals = p3.from_mont(data).astype(np.int64)            # (16, n) canonical
    cyc = int(seg.cycles)
    tr = {k: vals[c, :cyc] | vals[c + 1, :cyc] << 16 for k, c in
          (("pc", PC_LO), ("next", NX_LO), ("ins", INS_LO), ("a", A_LO), ("b", B_LO), ("res", RES_LO))}
    tr["wr"] = vals[WR, :cyc]
    return tr, vals.shape[1], int(tr["pc"].min()) if cyc else 0, int(tr["pc"].max()) if cyc else 0


def shard_publics(seg, init, final, final_expected):
    """what every chip set's shard_tables ends with: the final registers are the executor's (final_expected, unless None)
    -> (cpu public values, register public values)"""
    if final_expected is not None and not np.array_equal(final, _u(final_expected)):
        raise ValueError("segment %d: the register accesses do not end in the executor's registers" % seg.index)
    pub_cpu = np.array([seg.start_pc & 0xFFFF, seg.start_pc >> 16, seg.end_pc & 0xFFFF, seg.end_pc >> 16], dtype=np.int64)
    return pub_cpu, register_publics(init, final)


def shard_tables(seg, data, init, final_expected, ecalls):
    """the five canonical tables of one executed segment -> ([cpu, program, register, byte, range] canonical int64 arrays,
    cpu public values, register public values)"""
    tr, n, pc_lo, pc_hi = trace_of(seg, data)
    cpu, final, final_ts, hist, byte_mult = cpu_rows(tr, n, seg.end_pc, init, ecalls)
    pubs = shard_publics(seg, init, final, final_expected)
    prog = program_table_for(tr["pc"], tr["ins"], pc_lo, pc_hi)
    rng = np.stack([np.arange(1 << 16, dtype=np.int64), hist], axis=1)
    return ([cpu, prog, register_rows(init, final, final_ts), byte_rows(byte_mult), rng],) + pubs


def bus_balance(tables_canon, airs_):
    """multiset equality per bus over one shard's canonical tables: -> {bus: Counter of tuple -> sends - receives} with
    the zero entries dropped (an empty dict per bus: the bus balances)"""
    from collections import Counter
    from . import p3
    out = {}
    for t, air in zip(tables_canon, airs_):
        t = np.asarray(t, dtype=np.int64)
        for it in air.interactions:
            m = np.full(t.shape[0], it.mult, dtype=np.int64) if it.mult_is_const else t[:, it.mult]
            sign = 1 if it.kind == p3.SEND else -1
            c = out.setdefault(it.bus, Counter())
            nz = np.nonzero(m % P)[0]
            vals = t[np.ix_(nz, it.value_cols)] % P
            for row, mm in zip(map(tuple, vals.tolist()), m[nz].tolist()):
                c[row] = (c[row] + sign * mm) % P
    return {bus: {k: v for k, v in c.items() if v % P} for bus, c in out.items()}
