"""The rv32i-cf chip set: the rv32i chip set (rv32.py) with the control flow and the shifts constrained as well.  A strict
extension: the cpu table's columns 0..67 and the program table's columns 0..76 are rv32i's, written by rv32.py's code,
the cpu and program AIRs are rv32i's bodies (rv32.cpu_constraints / rv32.program_constraints) plus the constraints
below, the register, byte and range tables and AIRs are rv32i's.  Six tables per shard:

  cpu       one row per cycle (CPU_COLS columns): rv32i's 68, then the decoded control-flow and shift selectors with the
            branch / jump offset (looked up in the program table), the branch decision's difference / borrow / equality
            columns, the next pc's carries, and the shift's amount decomposition, byte lookups and assembled result
  program   rv32i's 77 columns, then the same decoded fields, proven from the word's 32 bits
  register, byte, range   rv32i's
  shift     2^12 rows (2304 used): (k, x, lo, hi) with x 2^k = lo + 256 hi for k in 0..8, x in 0..255, proven from bit
            decompositions; receives SHIFT tuples

What the new constraints establish, on active rows:
  next pc    nx = pc + imm_B on a taken branch, pc + imm_J on JAL, (rs1 + imm_I) & ~1 on JALR (the dropped bit is the
             boolean DROP, nx_lo = 2 NXH with NXH in RANGE16), pc + 4 on every other row, all mod 2^32 (carries NC0, NC1)
  branches   TAKEN is the funct3 condition on the rs1 / rs2 values the REGISTER bus binds: a - b = BD (mod 2^32) with BD's
             limbs in RANGE16 and BC1 its borrow (BLTU / BGEU); a == b iff BD_LO + BD_HI = 0 (< 2^17, no wrap), tested
             through INV; BLT / BGE from rv32i's SA / SB / SNE and BC1, with SA_CHK / SB_CHK sent to RANGE16 on those
             rows (multiplicities M_SA / M_SB)
  shifts     SLL / SRL / SRA and their immediate forms: the amount s = k + 8q (k = three bits, q one-hot over 0..3) is the
             shamt field (RS2) or b_lo - 32 T with T in RANGE16; every byte of a' (a, complemented for SRA of a negative
             a, FILL = IS_SRA * SA with SA_CHK in RANGE16) is looked up once in the shift table with SK = k (left) or 8 - k
             (right); the result bytes are assembled from the lo / hi parts and selected by q (U), complemented back
             for FILL (V), and equal RES on rows that write rd
Every new multiplicity column (IS_BR, IS_SHIFT, M_SA, M_SB, IS_LINK for NXH) is 0 on padding rows.  RV32I is then
constrained except the loads and stores (LB / LH / LW / LBU / LHU / SB / SH / SW: memory stays free) and the a0 an ecall
leaves; the program table is still not bound to the ELF.

`shard_tables` builds every table of a segment in numpy (rv32_sets.p3_rv32cf_shards): the yardstick for
rk_exec_rv32cf_shard_device."""
import numpy as np

from . import rv32
from .rv32 import (ACTIVE, A_HI, A_LO, B_HI, B_LO, IMM_HI, IMM_LO, IS_IMM, IS_LINK, NX_HI, NX_LO, PC_HI, PC_LO, RES_HI,
                   RES_LO, RS2, SA, SA_CHK, SB, SB_CHK, SNE, WR, lin)
from .p3_trace import p3_range_air
from .segment import P

BUS_SHIFT = 7

# ---- cpu columns past rv32i's 68: first the fields looked up in the program table (in the program table's order)
(IS_JAL, IS_BEQ, IS_BNE, IS_BLT, IS_BGE, IS_BLTU, IS_BGEU, JIMM_LO, JIMM_HI, IS_SLL, IS_SRL, IS_SRA) = range(68, 80)
(IS_BR, TAKEN, BD_LO, BD_HI, BC0, BC1, EQ, INV, M_SA, M_SB, NC0, NC1, DROP, NXH) = range(80, 94)
IS_SHIFT, KB, Q, SK, T, FILL, U_LO, U_HI, V_LO, V_HI = 94, 95, 98, 102, 103, 104, 105, 106, 107, 108
SX, SLO, SHI = 109, 113, 117    # bytes of a' (the shifted operand), the shift table's lo / hi of each (4 each)
CPU_COLS = 121
PROGRAM_TUPLE = rv32.PROGRAM_TUPLE + list(range(IS_JAL, IS_SRA + 1))
BRANCH_F3 = (0, 1, 4, 5, 6, 7)  # funct3 of IS_BEQ .. IS_BGEU

# ---- program columns past rv32i's 77: the same twelve fields
P_EXT = rv32.PROGRAM_COLS
PROGRAM_COLS = P_EXT + 12

# ---- shift table columns
H_K, H_X, H_LO, H_HI, H_MULT, H_XB, H_KS, H_VB = 0, 1, 2, 3, 4, 5, 13, 22
SHIFT_COLS, SHIFT_LOG_ROWS, SHIFT_USED = 38, 12, 9 * 256

RANGE_SENDS = rv32.RANGE_SENDS + [(BD_LO, IS_BR), (BD_HI, IS_BR), (NXH, IS_LINK), (T, IS_SHIFT), (SA_CHK, M_SA),
                                  (SB_CHK, M_SB)]


def _shift_bytes(lo, hi):
    """the four result bytes per q of a left (u) and a right (v) shift from the shift table's lo / hi parts"""
    u = [lo[0], lo[1] + hi[0], lo[2] + hi[1], lo[3] + hi[2]]
    v = [hi[0] + lo[1], hi[1] + lo[2], hi[2] + lo[3], hi[3]]
    left = [[u[i - q] if i >= q else None for i in range(4)] for q in range(4)]
    right = [[v[i + q] if i + q < 4 else None for i in range(4)] for q in range(4)]
    return left, right


def _limb(bytes2):
    lo, hi = bytes2
    if lo is None and hi is None:
        return None
    if lo is None:
        return hi * 256
    return lo if hi is None else lo + hi * 256


def cpu_air(ext_w=None):
    """-> the cpu Air; its `constraint_names` maps the name of each new constraint to its index (the k of
    Air.check_trace's (row, k))"""
    from . import p3
    b = p3.AirBuilder(CPU_COLS, rv32.N_PUBLIC_CPU, p3.EXT_W if ext_w is None else ext_w)
    names = cpu_constraints(b, PROGRAM_TUPLE)
    air = b.build()
    air.constraint_names = names
    return air


def cpu_constraints(b, program_tuple):
    """the rv32i-cf cpu AIR's interactions and constraints into builder b (the rv32im cpu table appends its columns,
    rv32im.py); program_tuple: the cpu columns looked up in the program table -> {name: constraint index}"""
    from . import p3
    rv32.cpu_constraints(b, program_tuple)
    L = b.local
    names = {}

    def named(name, x):
        names[name] = sum(1 for step in b.steps if step[0] == p3.ASSERT_ZERO)
        b.assert_zero(x)

    for k in range(4):
        b.send(BUS_SHIFT, [SK, SX + k, SLO + k, SHI + k], mult=IS_SHIFT, mult_is_const=False)
    for c, m in RANGE_SENDS[len(rv32.RANGE_SENDS):]:
        b.send(rv32.BUS_RANGE16, [c], mult=m, mult_is_const=False)
    active, link, jal = L(ACTIVE), L(IS_LINK), L(IS_JAL)
    beq, bne, blt, bge, bltu, bgeu = (L(c) for c in range(IS_BEQ, IS_BGEU + 1))
    sll, srl, sra = L(IS_SLL), L(IS_SRL), L(IS_SRA)
    kb, q = [L(KB + i) for i in range(3)], [L(Q + i) for i in range(4)]
    for col in [BC0, BC1, NC0, NC1, DROP] + [KB + i for i in range(3)] + [Q + j for j in range(4)]:
        named("bool %d" % col, L(col) * (L(col) - 1))
    # the multiplicity columns: sums of the looked-up selectors, 0 on padding rows
    br, shift = L(IS_BR), L(IS_SHIFT)
    b.assert_eq(br, beq + bne + blt + bge + bltu + bgeu)
    b.assert_eq(shift, sll + srl + sra)
    named("m_sb", L(M_SB) - blt - bge)
    named("m_sa", L(M_SA) - blt - bge - sra)
    for c in (IS_BR, IS_SHIFT, M_SA, M_SB, IS_LINK):
        b.assert_zero((1 - active) * L(c))
    # branch decision: a = BD + b (mod 2^32), BC1 the borrow of a - b; EQ = [BD_LO + BD_HI = 0]
    a_lo, a_hi, b_lo, b_hi = L(A_LO), L(A_HI), L(B_LO), L(B_HI)
    bc0, bc1, eq = L(BC0), L(BC1), L(EQ)
    b.assert_zero(br * (L(BD_LO) + b_lo - a_lo - bc0 * 65536))
    b.assert_zero(br * (L(BD_HI) + b_hi + bc0 - a_hi - bc1 * 65536))
    z = L(BD_LO) + L(BD_HI)
    named("eq_inv", br * (z * L(INV) - 1 + eq))
    named("eq_zero", br * z * eq)
    lt_s = L(SA) * (1 - L(SB)) + (1 - L(SNE)) * bc1           # operand b is rs2's value on branch rows (IS_IMM = 0)
    taken = L(TAKEN)
    named("decision", taken - (beq * eq + bne * (1 - eq) + blt * lt_s + bge * (1 - lt_s) + bltu * bc1 + bgeu * (1 - bc1)))
    # next pc = base + offset (mod 2^32): base rs1's value on JALR rows, pc otherwise; JALR drops the sum's low bit
    jalr = link - jal
    jump = taken + jal
    four = 1 - taken - link
    named("next_lo", active * (L(PC_LO) + jalr * (a_lo - L(PC_LO)) + jump * L(JIMM_LO) + jalr * L(IMM_LO) + four * 4
                               - L(NX_LO) - L(DROP) - L(NC0) * 65536))
    named("next_hi", active * (L(PC_HI) + jalr * (a_hi - L(PC_HI)) + jump * L(JIMM_HI) + jalr * L(IMM_HI) + L(NC0)
                               - L(NX_HI) - L(NC1) * 65536))
    b.assert_zero(L(DROP) * (1 - jalr))
    named("nx_even", link * (L(NX_LO) - L(NXH) * 2))             # the target's low bit is 0 (NXH < 2^16)
    # shifts: s = k + 8 q, bound to the shamt field or to b_lo mod 32
    k = lin([(kb[i], 1 << i) for i in range(3)])
    s = k + lin([(q[j], 8 * j) for j in range(1, 4)])
    imm = L(IS_IMM)
    b.assert_zero(shift * (q[0] + q[1] + q[2] + q[3] - 1))
    named("amount", shift * (imm * (L(RS2) - s) + (1 - imm) * (b_lo - s - L(T) * 32)))
    sr = srl + sra
    b.assert_eq(L(SK), k + sr * (8 - k * 2))
    fill = L(FILL)
    b.assert_eq(fill, sra * L(SA))
    for lo_col, (x0, x1) in ((A_LO, (SX, SX + 1)), (A_HI, (SX + 2, SX + 3))):
        xv = L(x0) + L(x1) * 256
        b.assert_zero(shift * (L(lo_col) - xv - fill * (65535 - xv * 2)))
    left, right = _shift_bytes([L(SLO + j) for j in range(4)], [L(SHI + j) for j in range(4)])
    for half, u_col, v_col, res_col in ((0, U_LO, V_LO, RES_LO), (1, U_HI, V_HI, RES_HI)):
        terms = None
        for j in range(4):
            lt, rt = _limb(left[j][2 * half:2 * half + 2]), _limb(right[j][2 * half:2 * half + 2])
            part = None
            if lt is not None:
                part = sll * lt
            if rt is not None:
                part = sr * rt if part is None else part + sr * rt
            if part is not None:
                part = q[j] * part
                terms = part if terms is None else terms + part
        b.assert_eq(L(u_col), terms)
        b.assert_eq(L(v_col), L(u_col) + fill * (65535 - L(u_col) * 2))
        named("result %d" % half, shift * L(WR) * (L(res_col) - L(v_col)))
    return names


def program_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(PROGRAM_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    program_constraints(b, list(range(20)) + list(range(P_EXT, PROGRAM_COLS)))
    return b.build()


def program_constraints(b, tuple_cols):
    """the rv32i-cf program AIR's interaction and constraints into builder b (the rv32im program table appends its
    columns, rv32im.py); tuple_cols: the program columns the PROGRAM bus receives"""
    rv32.program_constraints(b, tuple_cols)
    L = b.local
    bit = [L(rv32.P_BITS + i) for i in range(32)]
    opc = [L(rv32.P_OPC + k) for k in range(11)]
    f3 = [L(rv32.P_F3 + j) for j in range(8)]
    mult, branch, jal = L(rv32.P_MULT), opc[rv32.O_BRANCH], opc[rv32.O_JAL]
    c = lambda col: L(P_EXT + col - IS_JAL)
    b.assert_eq(c(IS_JAL), jal)
    for col, j in zip(range(IS_BEQ, IS_BGEU + 1), BRANCH_F3):
        b.assert_eq(c(col), branch * f3[j])
    b.assert_zero(mult * branch * (f3[2] + f3[3]))            # the executor traps those words
    b_lo = lin([(bit[7 + i], 1 << i) for i in range(1, 5)] + [(bit[20 + i], 1 << i) for i in range(5, 11)]
               + [(bit[7], 1 << 11), (bit[31], 65536 - 4096)])
    j_lo = lin([(bit[20 + i], 1 << i) for i in range(1, 11)] + [(bit[20], 1 << 11)] + [(bit[i], 1 << i) for i in range(12, 16)])
    j_hi = lin([(bit[16 + i], 1 << i) for i in range(4)] + [(bit[31], 65536 - 16)])
    b.assert_eq(c(JIMM_LO), branch * b_lo + jal * j_lo)
    b.assert_eq(c(JIMM_HI), branch * (bit[31] * 65535) + jal * j_hi)
    alu = L(rv32.P_OPR) + opc[rv32.O_OPIMM]
    b.assert_eq(c(IS_SLL), alu * f3[1])
    b.assert_eq(c(IS_SRL), alu * f3[5] * (1 - bit[30]))
    b.assert_eq(c(IS_SRA), alu * f3[5] * bit[30])
    # funct7 of a looked-up shift word: 0, or 0x20 for SRL / SRA (bit 25 is shamt[5] of an immediate shift)
    high = lin([(bit[i], 1) for i in (25, 26, 27, 28, 29, 31)])
    b.assert_zero(mult * (c(IS_SLL) + c(IS_SRL) + c(IS_SRA)) * high)
    b.assert_zero(mult * c(IS_SLL) * bit[30])


def shift_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(SHIFT_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    L = b.local
    b.receive(BUS_SHIFT, [H_K, H_X, H_LO, H_HI], mult=H_MULT, mult_is_const=False)
    xb, ks, vb = [L(H_XB + i) for i in range(8)], [L(H_KS + j) for j in range(9)], [L(H_VB + i) for i in range(16)]
    for v in xb + ks + vb:
        b.assert_zero(v * (v - 1))
    b.assert_eq(lin([(v, 1) for v in ks]), b.const(1))
    b.assert_eq(L(H_K), lin([(ks[j], j) for j in range(1, 9)]))
    b.assert_eq(L(H_X), lin([(xb[i], 1 << i) for i in range(8)]))
    b.assert_eq(L(H_LO), lin([(vb[i], 1 << i) for i in range(8)]))
    b.assert_eq(L(H_HI), lin([(vb[8 + i], 1 << i) for i in range(8)]))
    b.assert_eq(lin([(vb[i], 1 << i) for i in range(16)]), L(H_X) * lin([(ks[j], 1 << j) for j in range(9)]))
    return b.build()


def airs(ext_w=None):
    """-> (cpu, program, register, byte, range, shift): the AIRs of one rv32i-cf shard, in table order"""
    return (cpu_air(ext_w), program_air(ext_w), rv32.register_air(ext_w), rv32.byte_air(ext_w), p3_range_air(ext_w),
            shift_air(ext_w))


# ------------------------------------------------------------------------------------------------ numpy witness
def decode(ins):
    """the twelve appended fields of instruction words (int64 array) -> (n, 12) int64, in PROGRAM_TUPLE order"""
    ins = np.asarray(ins, dtype=np.int64) & 0xFFFFFFFF
    d = rv32.decode(ins)
    bits, opc, f3 = d["bits"], d["opc"], d["f3"]
    branch, jal = opc[:, rv32.O_BRANCH], opc[:, rv32.O_JAL]
    bimm = (bits[:, 31] << 12 | bits[:, 7] << 11 | ((ins >> 25) & 0x3F) << 5 | ((ins >> 8) & 0xF) << 1)
    bimm = np.where(bits[:, 31] == 1, bimm | 0xFFFFE000, bimm)
    jimm = (bits[:, 31] << 20 | ((ins >> 12) & 0xFF) << 12 | bits[:, 20] << 11 | ((ins >> 21) & 0x3FF) << 1)
    jimm = np.where(bits[:, 31] == 1, jimm | 0xFFE00000, jimm)
    off = branch * bimm + jal * jimm
    alu = d["opr"] + opc[:, rv32.O_OPIMM]
    cols = [jal] + [branch * f3[:, j] for j in BRANCH_F3] + [off & 0xFFFF, off >> 16, alu * f3[:, 1],
                                                             alu * f3[:, 5] * (1 - bits[:, 30]), alu * f3[:, 5] * bits[:, 30]]
    return np.stack(cols, axis=1)


def program_table_for(pcs, inss, pc_lo, pc_hi):
    """rv32.program_table_for with the twelve decoded fields appended"""
    base = rv32.program_table_for(pcs, inss, pc_lo, pc_hi)
    return np.concatenate([base, decode(base[:, 2] | base[:, 3] << 16)], axis=1)


def shift_rows(mult=None):
    n = 1 << SHIFT_LOG_ROWS
    r = np.arange(SHIFT_USED, dtype=np.int64)
    k, x = r >> 8, r & 255
    v = x << k
    t = np.zeros((n, SHIFT_COLS), dtype=np.int64)
    t[:, H_KS] = 1                                 # padding rows: (0, 0, 0, 0), a true tuple, with multiplicity 0
    t[:SHIFT_USED, H_KS] = 0
    t[:SHIFT_USED, H_K], t[:SHIFT_USED, H_X], t[:SHIFT_USED, H_LO], t[:SHIFT_USED, H_HI] = k, x, v & 255, v >> 8
    t[:SHIFT_USED, H_XB:H_XB + 8] = (x[:, None] >> np.arange(8)) & 1
    t[r, H_KS + k] = 1
    t[:SHIFT_USED, H_VB:H_VB + 16] = (v[:, None] >> np.arange(16)) & 1
    if mult is not None:
        t[:SHIFT_USED, H_MULT] = mult[:SHIFT_USED]
    return t


def cpu_rows(tr, n, end_pc, init, ecalls, strict=True):
    """rv32.cpu_rows with the columns of the control flow and the shifts appended -> (cpu table (n, CPU_COLS) int64,
    final values, final timestamps, RANGE16 histogram, BYTE multiplicities, SHIFT multiplicities).  strict: raise
    ValueError when a next pc or a written shift result is not the instruction's.  strict=False (the tests' forged
    traces): the witness follows what the trace claims, as a forger's would -- TAKEN says whether the trace went to the
    branch target, the carries are those of that next pc -- while the decision's and the shift's own columns are the
    true ones"""
    base, final, final_ts, hist, byte_mult = rv32.cpu_rows(tr, n, end_pc, init, ecalls)
    cyc = tr["pc"].size
    t = np.zeros((n, CPU_COLS), dtype=np.int64)
    t[:, :rv32.CPU_COLS] = base
    M = 0xFFFFFFFF
    pc, ins, a, bv, nxt = (np.asarray(tr[k], dtype=np.int64) for k in ("pc", "ins", "a", "b", "next"))
    res = base[:cyc, RES_LO] | base[:cyc, RES_HI] << 16
    dec = decode(ins)
    d = rv32.decode(ins)
    c = {IS_JAL + j: dec[:, j] for j in range(12)}
    sel = lambda col: c[col]
    br = sum(sel(col) for col in range(IS_BEQ, IS_BGEU + 1))
    shift = sel(IS_SLL) + sel(IS_SRL) + sel(IS_SRA)
    # branch decision
    sa, sb = a >> 31, bv >> 31
    lt_u = (a < bv).astype(np.int64)
    lt_s = np.where(sa != sb, sa, lt_u)
    eqv = (a == bv).astype(np.int64)
    cond = sum(sel(col) * v for col, v in zip(range(IS_BEQ, IS_BGEU + 1), (eqv, 1 - eqv, lt_s, 1 - lt_s, lt_u, 1 - lt_u)))
    dd = (a - bv) & M
    z = br * ((dd & 0xFFFF) + (dd >> 16))
    inv = np.array([pow(int(v), P - 2, P) if v else 0 for v in z.tolist()], dtype=np.int64)
    jimm = sel(JIMM_LO) | sel(JIMM_HI) << 16
    taken = cond if strict else br * (nxt == (pc + jimm) & M)
    c.update({IS_BR: br, TAKEN: taken, BD_LO: br * (dd & 0xFFFF), BD_HI: br * (dd >> 16),
              BC0: br * ((a & 0xFFFF) < (bv & 0xFFFF)), BC1: br * lt_u, EQ: br * eqv, INV: inv,
              M_SA: sel(IS_BLT) + sel(IS_BGE) + sel(IS_SRA), M_SB: sel(IS_BLT) + sel(IS_BGE)})
    # next pc
    jal, link = sel(IS_JAL), d["is_link"]
    jalr = link - jal
    base_v = np.where(jalr == 1, a, pc)
    off_v = np.where(jalr == 1, d["imm"], np.where(taken + jal > 0, jimm, 4))
    nc0 = ((base_v & 0xFFFF) + (off_v & 0xFFFF)) >> 16
    nc1 = ((base_v >> 16) + (off_v >> 16) + nc0) >> 16
    s = (base_v + off_v) & M
    drop = jalr * (s & 1)
    if strict and not np.array_equal(s - drop, nxt):
        raise ValueError("a next pc is not the one the instruction names")
    c.update({NC0: nc0, NC1: nc1, DROP: drop, NXH: link * ((nxt & 0xFFFF) >> 1)})
    # shifts
    imm = d["is_imm"]
    amt = shift * np.where(imm == 1, d["rs2"], bv & 31)
    k, q = amt & 7, amt >> 3
    sr = sel(IS_SRL) + sel(IS_SRA)
    fill = sel(IS_SRA) * sa
    ap = a ^ (fill * M)
    sk = shift * (k + sr * (8 - 2 * k))
    u = shift * np.where(sel(IS_SLL) == 1, (ap << amt) & M, ap >> amt)
    v = u ^ (fill * M)
    if strict and (shift * d["wr"] * (v - res)).any():
        raise ValueError("a shift result is not the one the instruction names")
    c.update({IS_SHIFT: shift, SK: sk, T: shift * (1 - imm) * ((bv & 0xFFFF) >> 5), FILL: fill,
              U_LO: u & 0xFFFF, U_HI: u >> 16, V_LO: v & 0xFFFF, V_HI: v >> 16})
    for i in range(3):
        c[KB + i] = shift * ((k >> i) & 1)
    for j in range(4):
        c[Q + j] = shift * (q == j)
        x = shift * ((ap >> (8 * j)) & 255)
        c[SX + j], c[SLO + j], c[SHI + j] = x, (x << sk) & 255, (x << sk) >> 8
    for col, val in c.items():
        t[:cyc, col] = val
    for col, m in RANGE_SENDS[len(rv32.RANGE_SENDS):]:
        on = t[:, m] != 0
        hist += np.bincount(t[on, col], minlength=1 << 16)[: 1 << 16]
    shift_mult = np.zeros(SHIFT_USED, dtype=np.int64)
    rows = t[t[:, IS_SHIFT] == 1]
    for j in range(4):
        shift_mult += np.bincount(rows[:, SK] << 8 | rows[:, SX + j], minlength=SHIFT_USED)
    return t, final, final_ts, hist, byte_mult, shift_mult


def shard_tables(seg, data, init, final_expected, ecalls):
    """the six canonical tables of one executed segment -> ([cpu, program, register, byte, range, shift] canonical int64
    arrays, cpu public values, register public values)"""
    tr, n, pc_lo, pc_hi = rv32.trace_of(seg, data)
    cpu, final, final_ts, hist, byte_mult, shift_mult = cpu_rows(tr, n, seg.end_pc, init, ecalls)
    pubs = rv32.shard_publics(seg, init, final, final_expected)
    prog = program_table_for(tr["pc"], tr["ins"], pc_lo, pc_hi)
    rng = np.stack([np.arange(1 << 16, dtype=np.int64), hist], axis=1)
    return ([cpu, prog, rv32.register_rows(init, final, final_ts), rv32.byte_rows(byte_mult), rng,
             shift_rows(shift_mult)],) + pubs
