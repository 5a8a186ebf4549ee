"""The rv32im chip set: the rv32i-cf chip set (rv32cf.py) with the M extension constrained as well.  A strict extension:
the cpu table's columns 0..120 and the program table's columns 0..88 are rv32i-cf's, written by rv32cf.py's code, the
cpu and program AIRs are rv32i-cf's bodies plus the constraints below, the register, byte, range and shift tables and
AIRs are rv32i-cf's.  Seven tables per shard:

  cpu       one row per cycle (CPU_COLS columns): rv32i-cf's 121, then the decoded M selectors IS_MUL .. IS_REMU and
            their sum IS_M (looked up in the program table), the op MOP = funct3 and the multiplicity M_W = IS_M WR
  program   rv32i-cf's 89 columns, then the same nine fields and three partial products of the funct7 test, proven
            from the word's 32 bits
  register, byte, range, shift   rv32i-cf's
  muldiv    2^max(MD_MIN_LOG, ceil(log2 count)) rows: one per cpu row with M_W = 1, in execution order, then padding
            rows of multiplicity 0; receives (op, a_lo, a_hi, b_lo, b_hi, res_lo, res_hi) on BUS_MULDIV

A cpu row with M_W = 1 sends (MOP, A, B, RES) on BUS_MULDIV: A and B are bound by the REGISTER bus and RES is the value
written to rd, so the send binds the written value to a muldiv row.  An M instruction into x0 writes nothing (WR = 0)
and sends nothing; RES stays 0 there as under rv32i.

A muldiv row proves C = X Y + Z (mod 2^64) over byte limbs, X, Y, Z sign-extended to 8 bytes by the bits EX, EY, EZ:
  MUL*      X = a, Y = b, Z = 0; RES = C's low word (MUL) or high word (MULH / MULHSU / MULHU); EX = SX on MULH / MULHSU,
            EY = SY on MULH
  DIV*/REM* X = q, Y = b, Z = r; C = a sign-extended by EC (signed ops); RES = q (DIV / DIVU) or r (REM / REMU); with
            b = 0 (BZ, from BINV as EQ in rv32cf.py): q = 2^32 - 1 (and r = a follows from C = a); with a = -2^31,
            b = -1 on DIV / REM (OVF, forced through OINV exactly then): q = -2^31, r = 0 and C's high word is free;
            otherwise |r| < |b| on the magnitudes BM / RM (two's complement by EY / EZ) and r = 0 or sign(r) = sign(a)
Soundness bounds: every byte of X, Y, Z, C is a byte through the byte table (AND of a pair, op 1) or, for the top byte
of each, the shift table (k = 1: x 2 = lo + 256 hi, hi the sign bit); the eight carries, BM, RM and the difference DL =
|b| - |r| - 1 are sent to RANGE16.  Convolution k: at most eight products of bytes, 8 * 255^2 + 255 + a carry < 2^16 is
< 2^20, and c_k + 256 carry_k < 2^24, so no sum wraps p.  The magnitude and bound sums are < 2^18, the overflow
distance DEV < 2^12.  |q b + r| < 2^63 for signed operands and q b + r < 2^64 for unsigned ones, so C = a (mod 2^64)
is an equation over the integers and q, r are the truncated quotient and remainder.  The multiplicity MULT is boolean,
the sum of the one-hot op selectors, and once 0 stays 0 down the table.

`shard_tables` builds every table of a segment in numpy (rv32_sets.p3_rv32im_shards): the yardstick for
rk_exec_rv32im_shard_device."""
import numpy as np

from . import rv32, rv32cf
from .rv32 import A_HI, A_LO, B_HI, B_LO, RES_HI, RES_LO, WR, lin
from .p3_trace import p3_range_air
from .segment import P

BUS_MULDIV = 8
M_OPS = ("mul", "mulh", "mulhsu", "mulhu", "div", "divu", "rem", "remu")     # funct3 order
O_MUL, O_MULH, O_MULHSU, O_MULHU, O_DIV, O_DIVU, O_REM, O_REMU = range(8)

# ---- cpu columns past rv32i-cf's 121: the nine looked-up fields, then the op and the multiplicity
IS_MUL = rv32cf.CPU_COLS                     # IS_MUL + j: the op of funct3 j (M_OPS order)
IS_M, MOP, M_W = IS_MUL + 8, IS_MUL + 9, IS_MUL + 10
CPU_COLS = IS_MUL + 11
PROGRAM_TUPLE = rv32cf.PROGRAM_TUPLE + list(range(IS_MUL, IS_M + 1))

# ---- program columns past rv32i-cf's 89: the nine fields, then the partial products of the funct7 test
P_EXT = rv32cf.PROGRAM_COLS
P_F7 = P_EXT + 9
PROGRAM_COLS = P_EXT + 12

# ---- muldiv columns
D_SEL, D_MULT, D_OP, D_A_LO, D_A_HI, D_B_LO, D_B_HI, D_R_LO, D_R_HI, D_ONE = 0, 8, 9, 10, 11, 12, 13, 14, 15, 16
D_X, D_Y, D_Z, D_C, D_CY = 17, 21, 25, 29, 37                 # bytes of X, Y, Z (4 each), C (8), carries (8)
D_S, D_L, D_E = 45, 49, 53                                     # sign bit, shift-table lo part, extension bit: of X Y Z C
D_AND = 57                                                     # the AND of each byte pair (8)
D_BZ, D_BINV, D_OVF, D_OINV = 65, 66, 67, 68
D_BM_LO, D_BM_HI, D_KB, D_RM_LO, D_RM_HI, D_KR, D_DL_LO, D_DL_HI, D_K0 = range(69, 78)
MD_COLS = 78
MD_MIN_LOG = 1               # the smallest height the prover accepts (a degree-3 AIR's quotient in two chunks)
# the bytes checked through the byte table, in pairs (the top byte of X, Y, Z and C goes through the shift table)
BYTE_PAIRS = [(D_X, D_X + 1), (D_X + 2, D_Y), (D_Y + 1, D_Y + 2), (D_Z, D_Z + 1), (D_Z + 2, D_C), (D_C + 1, D_C + 2),
              (D_C + 4, D_C + 5), (D_C + 6, D_C + 7)]
SIGN_BYTES = [D_X + 3, D_Y + 3, D_Z + 3, D_C + 3]
RANGE_COLS = [D_CY + k for k in range(8)] + [D_BM_LO, D_BM_HI, D_RM_LO, D_RM_HI, D_DL_LO, D_DL_HI]
MD_TUPLE = [D_OP, D_A_LO, D_A_HI, D_B_LO, D_B_HI, D_R_LO, D_R_HI]


def _namer(b, names):
    from . import p3

    def named(name, x):
        names[name] = sum(1 for step in b.steps if step[0] == p3.ASSERT_ZERO)
        b.assert_zero(x)
    return named


def cpu_air(ext_w=None):
    """-> the cpu Air: rv32i-cf's body (and its named constraints) plus the M selectors' send"""
    from . import p3
    b = p3.AirBuilder(CPU_COLS, rv32.N_PUBLIC_CPU, p3.EXT_W if ext_w is None else ext_w)
    names = cpu_constraints(b, PROGRAM_TUPLE)
    air = b.build()
    air.constraint_names = names
    return air


def cpu_constraints(b, program_tuple):
    """the rv32im cpu AIR's interactions and constraints into builder b (the rv32im-mem cpu table appends its columns,
    rv32mem.py); program_tuple: the cpu columns looked up in the program table -> {name: constraint index}"""
    names = rv32cf.cpu_constraints(b, program_tuple)
    named = _namer(b, names)
    L = b.local
    b.send(BUS_MULDIV, [MOP, A_LO, A_HI, B_LO, B_HI, RES_LO, RES_HI], mult=M_W, mult_is_const=False)
    sel = [L(IS_MUL + j) for j in range(8)]
    named("mop", L(MOP) - lin([(sel[j], j) for j in range(1, 8)]))
    named("is_m", L(IS_M) - lin([(s, 1) for s in sel]))
    named("m_w", L(M_W) - L(IS_M) * L(WR))       # WR is 0 on padding rows, so M_W is too
    return names


def program_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(PROGRAM_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    rv32cf.program_constraints(b, list(range(20)) + list(range(rv32cf.P_EXT, P_EXT)) + list(range(P_EXT, P_EXT + 9)))
    L = b.local
    bit = [L(rv32.P_BITS + i) for i in range(32)]
    f3 = [L(rv32.P_F3 + j) for j in range(8)]
    op = L(rv32.P_OPC + rv32.O_OP)
    f7a, f7b, f7c, is_m = L(P_F7), L(P_F7 + 1), L(P_F7 + 2), L(P_EXT + 8)
    # funct7 = 0000001: bit 25 set, bits 26..31 clear, in partial products of degree <= 3
    b.assert_eq(f7a, op * bit[25] * (1 - bit[26]))
    b.assert_eq(f7b, f7a * (1 - bit[27]) * (1 - bit[28]))
    b.assert_eq(f7c, f7b * (1 - bit[29]) * (1 - bit[30]))
    b.assert_eq(is_m, f7c * (1 - bit[31]))
    for j in range(8):
        b.assert_eq(L(P_EXT + j), is_m * f3[j])
    # an OP word with bit 25 set that a cpu row looks up is an M word (the executor traps the other funct7 values)
    b.assert_zero(L(rv32.P_MULT) * (op * bit[25] - is_m))
    return b.build()


def muldiv_air(ext_w=None):
    """-> the muldiv Air; its `constraint_names` maps the name of each constraint to its index"""
    from . import p3
    b = p3.AirBuilder(MD_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    L = b.local
    names = {}
    named = _namer(b, names)
    mult, one = L(D_MULT), L(D_ONE)
    b.receive(BUS_MULDIV, MD_TUPLE, mult=D_MULT, mult_is_const=False)
    for j, (u, v) in enumerate(BYTE_PAIRS):
        b.send(rv32.BUS_BYTE, [D_ONE, u, v, D_AND + j], mult=D_MULT, mult_is_const=False)     # op 1: AND
    for j, c in enumerate(SIGN_BYTES):
        b.send(rv32cf.BUS_SHIFT, [D_ONE, c, D_L + j, D_S + j], mult=D_MULT, mult_is_const=False)   # k = 1: the sign bit
    for c in RANGE_COLS:
        b.send(rv32.BUS_RANGE16, [c], mult=D_MULT, mult_is_const=False)
    sel = [L(D_SEL + j) for j in range(8)]
    for j in range(8):
        named("bool sel %d" % j, sel[j] * (sel[j] - 1))
    named("mult", mult - lin([(s, 1) for s in sel]))
    named("bool mult", mult * (mult - 1))
    b.when_transition().assert_zero((1 - mult) * b.next(D_MULT))
    names["padding"] = sum(1 for step in b.steps if step[0] == p3.ASSERT_ZERO) - 1
    named("op", L(D_OP) - lin([(sel[j], j) for j in range(1, 8)]))
    named("one", one - 1)
    mul, mulh, mulhsu, mulhu, div, divu, rem, remu = sel
    mul_any, mul_hi = mul + mulh + mulhsu + mulhu, mulh + mulhsu + mulhu
    divs, div_any = div + rem, div + divu + rem + remu
    x, y, z, c = ([L(base + k) for k in range(n)] for base, n in ((D_X, 4), (D_Y, 4), (D_Z, 4), (D_C, 8)))
    cy = [L(D_CY + k) for k in range(8)]
    sx, sy, sz, sc = (L(D_S + j) for j in range(4))
    ex, ey, ez, ec = (L(D_E + j) for j in range(4))
    half = lambda v, k: v[k] + v[k + 1] * 256
    # Y = b on every row
    named("y lo", L(D_B_LO) - half(y, 0))
    named("y hi", L(D_B_HI) - half(y, 2))
    # the sign extensions: of X on MULH / MULHSU / DIV / REM, of Y on MULH / DIV / REM, of Z and C on DIV / REM
    named("ext x", ex - (mulh + mulhsu + divs) * sx)
    named("ext y", ey - (mulh + divs) * sy)
    named("ext z", ez - divs * sz)
    named("ext c", ec - divs * sc)
    # C = X Y + Z (mod 2^64), byte by byte with the carries
    xe, ye, ze = x + [ex * 255] * 4, y + [ey * 255] * 4, z + [ez * 255] * 4
    for k in range(8):
        acc = lin([(xe[i] * ye[k - i], 1) for i in range(k + 1)]) + ze[k]
        if k:
            acc = acc + cy[k - 1]
        named("conv %d" % k, acc - c[k] - cy[k] * 256)
    # MUL*: X = a, Z = 0, the result the low or the high word of C
    named("mul a lo", mul_any * (L(D_A_LO) - half(x, 0)))
    named("mul a hi", mul_any * (L(D_A_HI) - half(x, 2)))
    for k in range(4):
        named("mul z %d" % k, mul_any * z[k])
    named("mul lo", mul * (L(D_R_LO) - half(c, 0)))
    named("mul lo hi", mul * (L(D_R_HI) - half(c, 2)))
    named("mulh lo", mul_hi * (L(D_R_LO) - half(c, 4)))
    named("mulh hi", mul_hi * (L(D_R_HI) - half(c, 6)))
    # DIV*/REM*: C = a (its high word the sign extension, except in the overflow case), the result q or r
    ovf, bz = L(D_OVF), L(D_BZ)
    named("div a lo", div_any * (L(D_A_LO) - half(c, 0)))
    named("div a hi", div_any * (L(D_A_HI) - half(c, 2)))
    for k in range(4, 8):
        named("div a ext %d" % k, (div_any - ovf) * (c[k] - ec * 255))
    named("div q lo", (div + divu) * (L(D_R_LO) - half(x, 0)))
    named("div q hi", (div + divu) * (L(D_R_HI) - half(x, 2)))
    named("rem r lo", (rem + remu) * (L(D_R_LO) - half(z, 0)))
    named("rem r hi", (rem + remu) * (L(D_R_HI) - half(z, 2)))
    # b = 0: BZ = [b_lo + b_hi = 0] (< 2^17, no wrap) on division rows; then q = 2^32 - 1
    bsum = L(D_B_LO) + L(D_B_HI)
    named("bool bz", bz * (bz - 1))
    named("bz div", bz * (1 - div_any))
    named("bz inv", div_any * (bsum * L(D_BINV) - 1 + bz))
    named("bz zero", bz * bsum)
    for k in range(4):
        named("div0 q %d" % k, bz * (x[k] - 255))
    # a = -2^31, b = -1 on DIV / REM: OVF = [DEV = 0], DEV a sum of non-negative terms; then q = -2^31, r = 0
    dev = lin([(c[k], 2) for k in range(3)] + [(255 - y[k], 2) for k in range(4)] + [(1 - sc, 2), (L(D_L + 3), 1)])
    named("bool ovf", ovf * (ovf - 1))
    named("ovf div", ovf * (1 - divs))
    named("ovf inv", divs * (dev * L(D_OINV) - 1 + ovf))
    named("ovf zero", ovf * dev)
    for k in range(4):
        named("ovf q %d" % k, ovf * (x[k] - (128 if k == 3 else 0)))
        named("ovf r %d" % k, ovf * z[k])
    # magnitudes: BM = |b| (two's complement when EY), RM = |r| (when EZ); KB / KR the carries of b + BM = 2^32
    kb, kr, k0 = L(D_KB), L(D_KR), L(D_K0)
    r_lo, r_hi = half(z, 0), half(z, 2)
    for name, v in (("bool kb", kb), ("bool kr", kr), ("bool k0", k0)):
        named(name, v * (v - 1))
    for tag, e, lo, hi, m_lo, m_hi, kk in (("b", ey, L(D_B_LO), L(D_B_HI), L(D_BM_LO), L(D_BM_HI), kb),
                                           ("r", ez, r_lo, r_hi, L(D_RM_LO), L(D_RM_HI), kr)):
        named("mag %s lo" % tag, (1 - e) * (m_lo - lo) + e * (lo + m_lo - kk * 65536))
        named("mag %s hi" % tag, (1 - e) * (m_hi - hi) + e * (hi + m_hi + kk - 65536))
    # |r| + 1 + DL = |b| with DL >= 0 (its limbs in RANGE16, K0 the carry) on division rows with b != 0
    live = div_any - bz
    named("rem bound lo", live * (L(D_RM_LO) + 1 + L(D_DL_LO) - L(D_BM_LO) - k0 * 65536))
    named("rem bound hi", live * (L(D_RM_HI) + L(D_DL_HI) + k0 - L(D_BM_HI)))
    # r = 0 or sign(r) = sign(a): a >= 0 -> r >= 0; a < 0 -> r < 0 or r = 0
    named("rem sign pos", (divs - ec) * ez)
    named("rem sign neg", ec * (1 - ez) * (L(D_RM_LO) + L(D_RM_HI)))
    air = b.build()
    air.constraint_names = names
    return air


def airs(ext_w=None):
    """-> (cpu, program, register, byte, range, shift, muldiv): the AIRs of one rv32im shard, in table order"""
    return (cpu_air(ext_w), program_air(ext_w), rv32.register_air(ext_w), rv32.byte_air(ext_w), p3_range_air(ext_w),
            rv32cf.shift_air(ext_w), muldiv_air(ext_w))


# ------------------------------------------------------------------------------------------------ numpy witness
def decode(ins):
    """the twelve appended program fields of instruction words (int64 array) -> (n, 12) int64: IS_MUL .. IS_REMU, IS_M,
    then the three partial products of the funct7 test"""
    ins = np.asarray(ins, dtype=np.int64) & 0xFFFFFFFF
    d = rv32.decode(ins)
    bits, op = d["bits"], d["opc"][:, rv32.O_OP]
    nb = lambda i: 1 - bits[:, i]
    f7a = op * bits[:, 25] * nb(26)
    f7b = f7a * nb(27) * nb(28)
    f7c = f7b * nb(29) * nb(30)
    is_m = f7c * nb(31)
    return np.stack([is_m * d["f3"][:, j] for j in range(8)] + [is_m, f7a, f7b, f7c], axis=1)


def program_table_for(pcs, inss, pc_lo, pc_hi):
    """rv32cf.program_table_for with the twelve fields appended"""
    base = rv32cf.program_table_for(pcs, inss, pc_lo, pc_hi)
    return np.concatenate([base, decode(base[:, 2] | base[:, 3] << 16)], axis=1)


def cpu_rows(tr, n, end_pc, init, ecalls, strict=True):
    """rv32cf.cpu_rows with the M columns appended -> (cpu table (n, CPU_COLS) int64, final values, final timestamps,
    RANGE16 histogram, BYTE multiplicities, SHIFT multiplicities, (op, a, b, res) of every row with M_W = 1)"""
    base, final, final_ts, hist, byte_mult, shift_mult = rv32cf.cpu_rows(tr, n, end_pc, init, ecalls, strict)
    cyc = tr["pc"].size
    t = np.zeros((n, CPU_COLS), dtype=np.int64)
    t[:, :rv32cf.CPU_COLS] = base
    dec = decode(np.asarray(tr["ins"], dtype=np.int64))[:, :9]
    t[:cyc, IS_MUL:IS_M + 1] = dec
    t[:cyc, MOP] = (dec[:, :8] * np.arange(8)).sum(axis=1)
    t[:, M_W] = t[:, IS_M] * t[:, WR]
    on = t[:, M_W] == 1
    a = t[on, A_LO] | t[on, A_HI] << 16
    b = t[on, B_LO] | t[on, B_HI] << 16
    res = t[on, RES_LO] | t[on, RES_HI] << 16
    return t, final, final_ts, hist, byte_mult, shift_mult, (t[on, MOP], a, b, res)


def muldiv_log_rows(count):
    lg = MD_MIN_LOG
    while (1 << lg) < count:
        lg += 1
    return lg


def _inv(v):
    return np.array([pow(int(x), P - 2, P) if x else 0 for x in np.asarray(v).tolist()], dtype=np.int64)


def muldiv_witness(op, a, b):
    """the muldiv rows' columns of ops (funct3) on 32-bit operands a, b -> (rows (m, MD_COLS) int64 with RES the true
    result, results)"""
    op, a, b = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (op, a, b))
    M = 0xFFFFFFFF
    m = op.size
    t = np.zeros((m, MD_COLS), dtype=np.int64)
    sel = (op[:, None] == np.arange(8)).astype(np.int64)
    is_mul, divs = op < 4, (op == O_DIV) | (op == O_REM)
    sgn_x = (op == O_MULH) | (op == O_MULHSU) | divs
    sgn_y = (op == O_MULH) | divs
    # division: unsigned and signed (truncated), with the b = 0 and overflow conventions
    bz = b == 0
    bb = np.where(bz, 1, b)
    qu, ru = np.where(bz, M, a // bb), np.where(bz, a, a % bb)
    sa_, sb_ = a - (a >> 31 << 32), b - (b >> 31 << 32)
    mag = np.abs(sa_) // np.where(bz, 1, np.abs(sb_))
    qs = np.where(bz, -1, np.where((sa_ < 0) != (sb_ < 0), -mag, mag))
    rs = sa_ - qs * sb_
    q, r = np.where(divs, qs, qu) & M, np.where(divs, rs, ru) & M
    x, z = np.where(is_mul, a, q), np.where(is_mul, 0, r)
    byt = lambda v, k: (v >> (8 * k)) & 255
    xb, yb, zb = ([byt(v, k) for k in range(4)] for v in (x, b, z))
    s = [v >> 31 for v in (x, b, z)]
    e = [sgn_x * s[0], sgn_y * s[1], divs * s[2]]
    xe, ye, ze = (v + [ee * 255] * 4 for v, ee in zip((xb, yb, zb), e))
    cb, cy, carry = [], [], np.zeros(m, dtype=np.int64)
    for k in range(8):
        acc = sum(xe[i] * ye[k - i] for i in range(k + 1)) + ze[k] + carry
        cb.append(acc & 255)
        carry = acc >> 8
        cy.append(carry)
    sc = cb[3] >> 7
    s.append(sc)
    e.append(divs * sc)
    lo_w = cb[0] | cb[1] << 8 | cb[2] << 16 | cb[3] << 24
    hi_w = cb[4] | cb[5] << 8 | cb[6] << 16 | cb[7] << 24
    res = np.where(op == O_MUL, lo_w, np.where(is_mul, hi_w, np.where((op == O_DIV) | (op == O_DIVU), q, r)))
    t[:, D_SEL:D_SEL + 8] = sel
    t[:, D_MULT], t[:, D_OP] = 1, op
    t[:, D_A_LO], t[:, D_A_HI], t[:, D_B_LO], t[:, D_B_HI] = a & 0xFFFF, a >> 16, b & 0xFFFF, b >> 16
    t[:, D_R_LO], t[:, D_R_HI], t[:, D_ONE] = res & 0xFFFF, res >> 16, 1
    for k in range(4):
        t[:, D_X + k], t[:, D_Y + k], t[:, D_Z + k] = xb[k], yb[k], zb[k]
    for k in range(8):
        t[:, D_C + k], t[:, D_CY + k] = cb[k], cy[k]
    for j, col in enumerate(SIGN_BYTES):
        t[:, D_S + j], t[:, D_E + j] = s[j], e[j]
        t[:, D_L + j] = (2 * t[:, col]) & 255
    for j, (u, v) in enumerate(BYTE_PAIRS):
        t[:, D_AND + j] = t[:, u] & t[:, v]
    div_any = ~is_mul
    t[:, D_BZ] = div_any & bz
    t[:, D_BINV] = div_any * _inv((b & 0xFFFF) + (b >> 16))
    t[:, D_OVF] = divs & (a == 0x80000000) & (b == M)
    dev = (2 * (cb[0] + cb[1] + cb[2]) + 2 * sum(255 - yb[k] for k in range(4)) + 2 * (1 - sc) + t[:, D_L + 3])
    t[:, D_OINV] = divs * _inv(dev)
    bm = np.where(e[1] == 1, (1 << 32) - b, b)
    rm = np.where(e[2] == 1, (1 << 32) - z, z)
    t[:, D_BM_LO], t[:, D_BM_HI], t[:, D_KB] = bm & 0xFFFF, bm >> 16, e[1] * ((b & 0xFFFF) != 0)
    t[:, D_RM_LO], t[:, D_RM_HI], t[:, D_KR] = rm & 0xFFFF, rm >> 16, e[2] * ((z & 0xFFFF) != 0)
    live = div_any & ~bz
    dl = np.where(live, bm - rm - 1, 0)
    t[:, D_DL_LO], t[:, D_DL_HI] = dl & 0xFFFF, dl >> 16
    t[:, D_K0] = live * (((rm & 0xFFFF) + 1 + (dl & 0xFFFF)) >> 16)
    return t, res


def muldiv_rows(sends, n_rows=None, strict=True):
    """the muldiv table of the (op, a, b, res) a shard's cpu rows send -> (table (n_rows, MD_COLS) int64, RANGE16
    counts, BYTE counts, SHIFT counts it adds).  n_rows None: 2^muldiv_log_rows(count).  strict: raise ValueError when
    a claimed result is not the op's; strict=False (the tests' forged traces): RES is the claimed result, every other
    column the true witness"""
    op, a, b, res = (np.asarray(v, dtype=np.int64).reshape(-1) for v in sends)
    m = op.size
    n_rows = 1 << muldiv_log_rows(m) if n_rows is None else n_rows
    rows, want = muldiv_witness(op, a, b)
    if strict and not np.array_equal(want, res):
        raise ValueError("an M result is not the one the instruction names")
    rows[:, D_R_LO], rows[:, D_R_HI] = res & 0xFFFF, res >> 16
    t = np.zeros((n_rows, MD_COLS), dtype=np.int64)
    t[:, D_ONE] = 1
    t[:m] = rows
    hist = np.zeros(1 << 16, dtype=np.int64)
    for c in RANGE_COLS:
        hist += np.bincount(rows[:, c], minlength=1 << 16)[: 1 << 16]
    byte_mult = np.zeros(3 << 16, dtype=np.int64)
    for j, (u, v) in enumerate(BYTE_PAIRS):
        byte_mult += np.bincount(rows[:, u] << 8 | rows[:, v], minlength=3 << 16)
    shift_mult = np.zeros(rv32cf.SHIFT_USED, dtype=np.int64)
    for col in SIGN_BYTES:
        shift_mult += np.bincount(256 + rows[:, col], minlength=rv32cf.SHIFT_USED)
    return t, hist, byte_mult, shift_mult


def shard_tables(seg, data, init, final_expected, ecalls):
    """the seven canonical tables of one executed segment -> ([cpu, program, register, byte, range, shift, muldiv]
    canonical int64 arrays, cpu public values, register public values)"""
    tr, n, pc_lo, pc_hi = rv32.trace_of(seg, data)
    cpu, final, final_ts, hist, byte_mult, shift_mult, sends = cpu_rows(tr, n, seg.end_pc, init, ecalls)
    pubs = rv32.shard_publics(seg, init, final, final_expected)
    md, h2, b2, s2 = muldiv_rows(sends)
    prog = program_table_for(tr["pc"], tr["ins"], pc_lo, pc_hi)
    rng = np.stack([np.arange(1 << 16, dtype=np.int64), hist + h2], axis=1)
    return ([cpu, prog, rv32.register_rows(init, final, final_ts), rv32.byte_rows(byte_mult + b2), rng,
             rv32cf.shift_rows(shift_mult + s2), md],) + pubs
