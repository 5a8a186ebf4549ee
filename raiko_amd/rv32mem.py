"""The rv32im-mem chip set: the rv32im-elf chip set (rv32elf.py) with loads, stores and memory constrained WITHIN A
SHARD.  A strict extension: keyed like rv32im-elf (the program, byte, range and shift tuples are preprocessed), the
register and muldiv tables and AIRs are rv32im's, the cpu table's columns 0..131 are rv32im's, written by rv32im.py's
code.  Nine tables per shard, rv32im-elf's seven in their order, then memop and memory:

  cpu       one row per cycle (CPU_COLS columns): rv32im's 132, then the six looked-up fields IS_LOAD, IS_STORE, MEM_OP
            (funct3 + 8 IS_STORE), MIMM_LO / MIMM_HI (imm_I of a load, imm_S of a store, sign-extended) and IS_SYS, then
            the multiplicities M_MEM = IS_LOAD WR + IS_STORE ACTIVE and N_ECW (N_ECW (1 - IS_SYS) = 0, 0 on padding
            rows), and EC_OP = 16 IS_SYS: interactions name columns, and EC_OP is the column that holds the op of the
            second send
  program   width 1 (the multiplicity), prep_width 48: rv32im-elf's 41 fields, the six above, VALID.  VALID is
            rv32im-elf's and additionally 0 on a LOAD word whose funct3 is not in {0, 1, 2, 4, 5} and on a STORE word
            whose funct3 is not in {0, 1, 2}.  Decode is trusted to setup, as under rv32im-elf: no program AIR
  register, byte, range, shift, muldiv   rv32im-elf's (the counts include the lookups of memop and memory)
  memop     2^max(1, ceil(log2 count)) rows: one per recorded access (executor.Execution.mem), in list order
  memory    2^max(1, ceil(log2 count)) rows: one per distinct touched word, in ascending address order: the BOUNDARY
            table (word address, initial value, final value, final timestamp)

A cpu row sends (MEM_OP, TSA, A, MIMM, B, RES) on BUS_MEMOP M_MEM times -- one per load that writes rd and per store --
and (EC_OP, TSA) N_ECW times: a tuple is read as padded with zeros (the permutation argument's random linear combination
of a short tuple is that of the long one with zeros), so the second is (16, TSA, 0, 0, 0, 0, 0, 0, 0, 0).  TSA = 3 row + 1
is the memory clock.  A load into x0 sends nothing (WR = 0), as an M instruction into x0.  The RES of a load, a free
cell up to rv32im-elf, is what the memop row gives back.

A memop row (MEMOP_COLS columns) is one of LB LH LW LBU LHU SB SH SW ECW (one-hot; MULT their sum, boolean, once 0
always 0).  It receives (OP, TS, A, MI, B, R) where OP is the selected op's code (0 1 2 4 5 8 9 10 16) and A .. R are 0 on
an ECW row.  Address: AD = A + MI mod 2^32 (carries K0, K1 boolean, AD's limbs in RANGE16; an ECW row's AD is free),
AD_LO = 4 WL + 2 O1 + O0 with O boolean and WL, WL4 = 4 WL in RANGE16 (so WL < 2^14); O0 = 0 on halfword rows, O0 = O1 =
0 on word and ECW rows; S0..S3 are the products of the O bits.  W / N are the bytes of the word before / after, BB those
of rs2 on store rows; all twelve are bytes through the byte table (AND pairs, muldiv's convention).  Loads: N = W; X =
sum S_k W[k] the selected byte, H0 / H1 the bytes of the half chosen by O1; TOP is X on LB, H1 on LH (0 otherwise) and SG
its top bit by the shift table's k = 1 row (x 2 = SL + 256 SG); R is X or the half extended by SG (LB / LH) or by zero
(LBU / LHU), the word on LW.  Stores: SB N[k] - W[k] = S_k (BB0 - W[k]); SH the same over the half chosen by O1 with BB0,
BB1; SW N = BB.  ECW: W and N are bounded bytes and otherwise free -- the freedom of "the a0 an ecall leaves", at an
ecall row's timestamp and as often as its N_ECW allows.

Memory argument on BUS_MEMORY, the register argument's form: a memop row receives (WL, AD_HI, W limbs, PTS) and sends
(WL, AD_HI, N limbs, TS), TS - PTS - 1 = DL + 2^14 DH with both in RANGE16: the difference is in [0, 2^30) and cannot
wrap p.  An ecall writes distinct words, so the strict inequality holds there too.  A memory row with REAL = 1 sends
(WL, WH, I limbs) -- timestamp 0 -- and receives (WL, WH, F limbs, FTS).  REAL is boolean, once 0 always 0.  A real row
bounds its own address: WL, WL4 = 4 WL and WH go to RANGE16, so WL < 2^14 and WH < 2^16.  FTS is not 0 on a real row
(FTS FINV = 1): a row with F = I and FTS = 0 would receive its own send and need no memop row at all.  Addresses
strictly increase, compared limb by limb so that no difference can wrap p: on a transition into a real row either
SAME = 1, WH' = WH and WL' - WL - 1 = GL, or SAME = 0 and WH' - WH - 1 = GH, with GL and GH in RANGE16.  The limbs are
below 2^16, so a difference lies in (-2^16, 2^16) and a negative one, p - d, is no 16-bit value.  (One comparison of
WL + 2^14 WH with a 30-bit gap would not do: p < 2^31, so p - d fits a 30-bit gap for large d.)  Two rows for one
address -- two parallel histories -- cannot be written.

STILL FREE: INIT of every touched word -- the boundary to the previous shard's FINAL and to the ELF's data image is not
proven; shard k + 1 may start a word from any value (rv32link.py binds it) -- what an ecall writes, and the a0 it leaves
(rv32io.py, io=True, binds both to the run's input and exit code; rv32commit.py, commit=True, binds the journal
RK_ECALL_COMMIT appends to).  The boundary table is what a cross-shard link (a digest, shared challenges or a Merkle image) would bind.

`shard_tables` builds a shard's nine traces in numpy: the yardstick for rk_exec_rv32mem_shard_device."""
import numpy as np

from . import rv32, rv32cf, rv32elf, rv32im
from .rv32 import ACTIVE, A_HI, A_LO, B_HI, B_LO, BUS_BYTE, BUS_RANGE16, RES_HI, RES_LO, TSA, WR, lin
from .rv32cf import BUS_SHIFT
from .segment import P

BUS_MEMOP, BUS_MEMORY = 9, 10
OPS = ("lb", "lh", "lw", "lbu", "lhu", "sb", "sh", "sw", "ecw")
OP_CODES = (0, 1, 2, 4, 5, 8, 9, 10, 16)
EC_CODE = 16
MIN_LOG = 1

# ---- cpu columns past rv32im's 132: the six looked-up fields, the two multiplicities, the op of the ecall send
IS_LOAD = rv32im.CPU_COLS
IS_STORE, MEM_OP, MIMM_LO, MIMM_HI, IS_SYS, M_MEM, N_ECW, EC_OP = range(IS_LOAD + 1, IS_LOAD + 9)
CPU_COLS = IS_LOAD + 9
PROGRAM_TUPLE = rv32im.PROGRAM_TUPLE + list(range(IS_LOAD, IS_SYS + 1))
P_VALID = len(PROGRAM_TUPLE)                      # preprocessed column 47
PROGRAM_PREP = P_VALID + 1
assert PROGRAM_PREP == 48

# ---- memop columns
G_SEL, G_MULT, G_OP, G_TS, G_A_LO, G_A_HI, G_MI_LO, G_MI_HI, G_B_LO, G_B_HI, G_R_LO, G_R_HI = 0, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19
G_AD_LO, G_AD_HI, G_K0, G_K1, G_WL, G_WL4, G_O0, G_O1 = range(20, 28)
G_S, G_W, G_N, G_BB = 28, 32, 36, 40              # position selectors, old / new / rs2 bytes (4 each)
G_X, G_H0, G_H1, G_TOP, G_SG, G_SL, G_ONE = range(44, 51)
G_AND = 51                                         # the AND of each byte pair (6)
G_PTS, G_DL, G_DH, G_W_LO, G_W_HI, G_N_LO, G_N_HI = range(57, 64)
MEMOP_COLS = 64
G_ECR, MEMOP_COLS_COMMIT, ECR_CODE = 64, 65, 17    # the commit form (rv32commit.py): a tenth selector, ECR, op 17
BYTE_PAIRS = [(G_W, G_W + 1), (G_W + 2, G_W + 3), (G_N, G_N + 1), (G_N + 2, G_N + 3), (G_BB, G_BB + 1), (G_BB + 2, G_BB + 3)]
RANGE_COLS = [G_AD_LO, G_AD_HI, G_WL, G_WL4, G_DL, G_DH]
MEMOP_TUPLE = [G_OP, G_TS, G_A_LO, G_A_HI, G_MI_LO, G_MI_HI, G_B_LO, G_B_HI, G_R_LO, G_R_HI]

# ---- memory (boundary) columns
B_WL, B_WH, B_I_LO, B_I_HI, B_F_LO, B_F_HI, B_FTS, B_REAL, B_GL, B_GH, B_WL4, B_SAME, B_FINV = range(13)
MEMORY_COLS = 13
MEMORY_RANGE = [B_GL, B_GH, B_WL, B_WL4, B_WH]      # sent to RANGE16 by every real row


# ------------------------------------------------------------------------------------------------ the AIRs
def cpu_air(ext_w=None):
    """-> the cpu Air: rv32im's body (and its named constraints) plus the two sends to memop"""
    from . import p3
    b = p3.AirBuilder(CPU_COLS, rv32.N_PUBLIC_CPU, p3.EXT_W if ext_w is None else ext_w)
    names = rv32im.cpu_constraints(b, PROGRAM_TUPLE)
    named = rv32im._namer(b, names)
    L = b.local
    b.send(BUS_MEMOP, [MEM_OP, TSA, A_LO, A_HI, MIMM_LO, MIMM_HI, B_LO, B_HI, RES_LO, RES_HI], mult=M_MEM, mult_is_const=False)
    b.send(BUS_MEMOP, [EC_OP, TSA], mult=N_ECW, mult_is_const=False)
    named("m_mem", L(M_MEM) - L(IS_LOAD) * L(WR) - L(IS_STORE) * L(ACTIVE))     # WR is 0 on padding rows
    named("n_ecw sys", L(N_ECW) * (1 - L(IS_SYS)))
    named("n_ecw padding", (1 - L(ACTIVE)) * L(N_ECW))
    named("ec_op", L(EC_OP) - L(IS_SYS) * EC_CODE)
    air = b.build()
    air.constraint_names = names
    return air


def program_air(ext_w=None):
    """rv32elf.program_air over the 48 preprocessed columns"""
    from . import p3
    b = p3.AirBuilder(1, 0, p3.EXT_W if ext_w is None else ext_w, prep_width=PROGRAM_PREP)
    b.receive(rv32.BUS_PROGRAM, [b.prep(c) for c in range(P_VALID)], mult=0, mult_is_const=False)
    b.assert_zero(b.local(0) * (1 - b.prep_local(P_VALID)))
    return b.build()


def memop_air(ext_w=None, io=False, commit=False):
    """-> the memop Air; its `constraint_names` maps the name of each constraint to its index.  io (rv32io.py): an ECW
    row obeys SW's constraints -- its tuple is an io word row's (16, TS, AD, 0, V, 0): AD = A + MI, N = BB = the bytes of
    B -- and nothing about it is free.  commit (rv32commit.py; with io): a 65th column, the selector of an ECR row (op 17),
    which obeys LW's constraints -- its tuple is a commit-word row's (17, TS, AD, 0, 0, V): word aligned, N = W, R = W"""
    from . import p3
    if commit and not io:
        raise ValueError("commit=True needs io=True")
    b = p3.AirBuilder(MEMOP_COLS_COMMIT if commit else MEMOP_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    L = b.local
    names = {}
    named = rv32im._namer(b, names)
    b.receive(BUS_MEMOP, MEMOP_TUPLE, mult=G_MULT, mult_is_const=False)
    b.receive(BUS_MEMORY, [G_WL, G_AD_HI, G_W_LO, G_W_HI, G_PTS], mult=G_MULT, mult_is_const=False)
    b.send(BUS_MEMORY, [G_WL, G_AD_HI, G_N_LO, G_N_HI, G_TS], mult=G_MULT, mult_is_const=False)
    for j, (u, v) in enumerate(BYTE_PAIRS):
        b.send(BUS_BYTE, [G_ONE, u, v, G_AND + j], mult=G_MULT, mult_is_const=False)       # op 1: AND
    b.send(BUS_SHIFT, [G_ONE, G_TOP, G_SL, G_SG], mult=G_MULT, mult_is_const=False)        # k = 1: the sign bit
    for c in RANGE_COLS:
        b.send(BUS_RANGE16, [c], mult=G_MULT, mult_is_const=False)
    sel = [L(G_SEL + j) for j in range(9)]
    lb, lh, lw, lbu, lhu, sb, sh, sw, ecw = sel
    mult = L(G_MULT)
    for j in range(9):
        named("bool sel %d" % j, sel[j] * (sel[j] - 1))
    ecr = L(G_ECR) if commit else None
    if commit:
        named("bool ecr", ecr * (ecr - 1))
    named("mult", mult - lin([(s, 1) for s in sel + ([ecr] if commit else [])]))
    named("bool mult", mult * (mult - 1))
    named("padding", b.is_transition() * (1 - mult) * b.next(G_MULT))
    named("op", L(G_OP) - lin([(s, c) for s, c in list(zip(sel[1:], OP_CODES[1:])) + ([(ecr, ECR_CODE)] if commit else [])]))
    named("one", L(G_ONE) - 1)
    for tag, c in (("k0", G_K0), ("k1", G_K1), ("o0", G_O0), ("o1", G_O1)):
        named("bool " + tag, L(c) * (L(c) - 1))
    # the address: A + MI = AD + 2^32 K1 (not on an ECW row, whose A and MI are 0 and whose address is the witness's)
    cpu_row = mult if io else mult - ecw
    named("addr lo", cpu_row * (L(G_A_LO) + L(G_MI_LO) - L(G_AD_LO) - L(G_K0) * 65536))
    named("addr hi", cpu_row * (L(G_A_HI) + L(G_MI_HI) + L(G_K0) - L(G_AD_HI) - L(G_K1) * 65536))
    o0, o1 = L(G_O0), L(G_O1)
    named("addr split", L(G_AD_LO) - L(G_WL) * 4 - o1 * 2 - o0)
    named("wl4", L(G_WL4) - L(G_WL) * 4)
    named("align half", (lh + lhu + sh) * o0)
    word_row = lw + sw + ecw + ecr if commit else lw + sw + ecw
    named("align word o0", word_row * o0)
    named("align word o1", word_row * o1)
    s = [L(G_S + k) for k in range(4)]
    named("s0", s[0] - (mult - o0) * (1 - o1))
    named("s1", s[1] - o0 * (1 - o1))
    named("s2", s[2] - (mult - o0) * o1)
    named("s3", s[3] - o0 * o1)
    w, n, bb = ([L(base + k) for k in range(4)] for base in (G_W, G_N, G_BB))
    half = lambda v, k: v[k] + v[k + 1] * 256
    named("w lo", L(G_W_LO) - half(w, 0))
    named("w hi", L(G_W_HI) - half(w, 2))
    named("n lo", L(G_N_LO) - half(n, 0))
    named("n hi", L(G_N_HI) - half(n, 2))
    store, load = sb + sh + sw, lb + lh + lw + lbu + lhu + ecr if commit else lb + lh + lw + lbu + lhu
    word_store = sw + ecw if io else sw
    named("b lo", (store + ecw if io else store) * (L(G_B_LO) - half(bb, 0)))
    named("b hi", (store + ecw if io else store) * (L(G_B_HI) - half(bb, 2)))
    # loads: the word stays, the result is the selected byte / half / word, extended
    for k in range(4):
        named("load keeps %d" % k, load * (n[k] - w[k]))
    x, h0, h1, top, sg = L(G_X), L(G_H0), L(G_H1), L(G_TOP), L(G_SG)
    named("x", x - lin([(s[k] * w[k], 1) for k in range(4)]))
    named("h0", h0 - w[0] - o1 * (w[2] - w[0]))
    named("h1", h1 - w[1] - o1 * (w[3] - w[1]))
    named("top", top - lb * x - lh * h1)
    r_lo, r_hi = L(G_R_LO), L(G_R_HI)
    named("lb lo", lb * (r_lo - x - sg * 0xFF00))
    named("lb hi", lb * (r_hi - sg * 0xFFFF))
    named("lbu lo", lbu * (r_lo - x))
    named("lbu hi", lbu * r_hi)
    named("lh lo", lh * (r_lo - h0 - h1 * 256))
    named("lh hi", lh * (r_hi - sg * 0xFFFF))
    named("lhu lo", lhu * (r_lo - h0 - h1 * 256))
    named("lhu hi", lhu * r_hi)
    word_load = lw + ecr if commit else lw
    named("lw lo", word_load * (r_lo - L(G_W_LO)))
    named("lw hi", word_load * (r_hi - L(G_W_HI)))
    # stores: the bytes the op names change to rs2's low bytes, the others stay
    for k in range(4):
        named("sb %d" % k, sb * (n[k] - w[k] - s[k] * (bb[0] - w[k])))
    for k in range(4):
        pick = o1 if k >= 2 else 1 - o1
        named("sh %d" % k, sh * (n[k] - w[k] - pick * (bb[k & 1] - w[k])))
    for k in range(4):
        named("sw %d" % k, word_store * (n[k] - bb[k]))
    # an ECW row matches the cpu row's short tuple (16, TS): the other eight cells are 0
    for c in () if io else MEMOP_TUPLE[2:]:
        named("ecw zero %d" % c, ecw * L(c))
    # the access comes after the one it follows
    named("ts", mult * (L(G_TS) - L(G_PTS) - 1 - L(G_DL) - L(G_DH) * 16384))
    air = b.build()
    air.constraint_names = names
    return air


def memory_air(ext_w=None):
    """-> the memory (boundary) Air; its `constraint_names` maps the name of each constraint to its index"""
    from . import p3
    b = p3.AirBuilder(MEMORY_COLS, 0, p3.EXT_W if ext_w is None else ext_w)
    L = b.local
    names = {}
    named = rv32im._namer(b, names)
    b.send(BUS_MEMORY, [B_WL, B_WH, B_I_LO, B_I_HI], mult=B_REAL, mult_is_const=False)          # at timestamp 0
    b.receive(BUS_MEMORY, [B_WL, B_WH, B_F_LO, B_F_HI, B_FTS], mult=B_REAL, mult_is_const=False)
    for c in MEMORY_RANGE:
        b.send(BUS_RANGE16, [c], mult=B_REAL, mult_is_const=False)
    real, same = L(B_REAL), L(B_SAME)
    named("bool real", real * (real - 1))
    named("padding", b.is_transition() * (1 - real) * b.next(B_REAL))
    named("wl4", L(B_WL4) - L(B_WL) * 4)
    named("touched", real * (L(B_FTS) * L(B_FINV) - 1))
    # the next real row's address is larger: the high limb grows, or it stays and the low limb grows
    named("bool same", same * (same - 1))
    into = b.is_transition() * b.next(B_REAL)
    named("same high", into * same * (b.next(B_WH) - L(B_WH)))
    named("ascending low", into * same * (b.next(B_WL) - L(B_WL) - 1 - L(B_GL)))
    named("ascending high", into * (1 - same) * (b.next(B_WH) - L(B_WH) - 1 - L(B_GH)))
    air = b.build()
    air.constraint_names = names
    return air


def airs(ext_w=None):
    """-> (cpu, program, register, byte, range, shift, muldiv, memop, memory): the AIRs of one rv32im-mem shard"""
    return (cpu_air(ext_w), program_air(ext_w), rv32.register_air(ext_w), rv32elf.byte_air(ext_w), rv32elf.range_air(ext_w),
            rv32elf.shift_air(ext_w), rv32im.muldiv_air(ext_w), memop_air(ext_w), memory_air(ext_w))


# ------------------------------------------------------------------------------------------------ numpy witness
def decode(ins):
    """the six appended program fields of instruction words (int64 array) -> ((n, 6) int64: IS_LOAD, IS_STORE, MEM_OP,
    MIMM_LO, MIMM_HI, IS_SYS; whether a cpu row may look the word up as far as these fields go: the funct3 of a LOAD
    / STORE word is one the executor runs)"""
    ins = np.asarray(ins, dtype=np.int64) & 0xFFFFFFFF
    d = rv32.decode(ins)
    load, store, sysw = d["opc"][:, rv32.O_LOAD], d["opc"][:, rv32.O_STORE], d["opc"][:, rv32.O_SYSTEM]
    f3 = (ins >> 12) & 7
    sign = ins >> 31
    imm_i = (ins >> 20) | sign * 0xFFFFF000
    imm_s = ((ins >> 25) << 5 | (ins >> 7) & 31) | sign * 0xFFFFF000
    mimm = load * imm_i + store * imm_s
    ok = 1 - load * (1 - np.isin(f3, (0, 1, 2, 4, 5))) - store * (1 - np.isin(f3, (0, 1, 2)))
    return np.stack([load, store, (load + store) * f3 + 8 * store, mimm & 0xFFFF, mimm >> 16, sysw], axis=1), ok


def prep_tables(image):
    """the four canonical preprocessed matrices -> (program (rows, 48), byte (2^18, 4), range (2^16, 1), shift (2^12, 4)):
    rv32elf.prep_tables with the six fields in front of VALID and VALID narrowed"""
    prog, byt, rng, sh = rv32elf.prep_tables(image)
    full = rv32elf.program_full_rows(image)
    fields, ok = decode(full[:, 2] | full[:, 3] << 16)
    return np.concatenate([prog[:, :rv32elf.P_VALID], fields, (prog[:, rv32elf.P_VALID] * ok)[:, None]], axis=1), byt, rng, sh


def preps_of(image):
    """prep_tables in table order: None for the tables without preprocessed columns"""
    prog, byt, rng, sh = prep_tables(image)
    return [None, prog, None, byt, rng, sh, None, None, None]


def log_rows(count):
    lg = MIN_LOG
    while (1 << lg) < count:
        lg += 1
    return lg


def _mem(mem):
    return np.asarray(mem, dtype=np.int64).reshape(-1, 4)


def cpu_rows(tr, n, end_pc, init, ecalls, mem, strict=True):
    """rv32im.cpu_rows with the nine columns appended; mem: the segment's access list (k, 4): cycle, word address, old
    word, new word -> rv32im.cpu_rows's tuple.  ValueError (strict) when the list is not in cycle order or is not one
    entry per load that writes rd and per store, and entries at ecall rows otherwise"""
    t0, final, final_ts, hist, byte_mult, shift_mult, sends = rv32im.cpu_rows(tr, n, end_pc, init, ecalls)
    cyc = tr["pc"].size
    t = np.zeros((n, CPU_COLS), dtype=np.int64)
    t[:, :rv32im.CPU_COLS] = t0
    fields, _ok = decode(np.asarray(tr["ins"], dtype=np.int64))
    t[:cyc, IS_LOAD:IS_SYS + 1] = fields
    t[:, M_MEM] = t[:, IS_LOAD] * t[:, WR] + t[:, IS_STORE] * t[:, ACTIVE]
    t[:, EC_OP] = EC_CODE * t[:, IS_SYS]
    mem = _mem(mem)
    if mem.shape[0] and ((np.diff(mem[:, 0]) < 0).any() or mem[-1, 0] >= cyc or mem[0, 0] < 0):
        raise ValueError("the access list is not in cycle order")
    per_cycle = np.bincount(mem[:, 0], minlength=n)
    t[:, N_ECW] = per_cycle * t[:, IS_SYS]
    if strict and not np.array_equal(per_cycle * (1 - t[:, IS_SYS]), t[:, M_MEM]):
        raise ValueError("the access list is not one entry per load that writes rd and per store")
    return t, final, final_ts, hist, byte_mult, shift_mult, sends


def memop_rows(cpu, mem, n_rows=None, io=False):
    """the memop table of an access list against the cpu table its rows answer -> (table (n_rows, MEMOP_COLS) int64,
    RANGE16 counts, BYTE counts, SHIFT counts it adds).  n_rows None: 2^log_rows(count).  OP, A, MI, B and R are the cpu
    row's (R the CLAIMED result: a forged one fails the op's result constraint), the word before and after are the
    list's, every other column the witness of the op on them.  io (rv32io.py): an ECW row is written as the store of the
    word it leaves: A its address, B and BB the word"""
    mem = _mem(mem)
    m = mem.shape[0]
    n_rows = 1 << log_rows(m) if n_rows is None else n_rows
    t = np.zeros((n_rows, MEMOP_COLS), dtype=np.int64)
    t[:, G_ONE] = 1
    M = 0xFFFFFFFF
    cyc, waddr, old, new = mem.T
    row = cpu[cyc]
    ecw = row[:, IS_SYS]
    live = 1 - ecw
    op = np.where(ecw == 1, EC_CODE, row[:, MEM_OP])
    sel = (op[:, None] == np.array(OP_CODES)).astype(np.int64)
    lb, lh, lw, lbu, lhu, sb, sh, sw, _e = sel.T
    a = live * (row[:, A_LO] | row[:, A_HI] << 16)
    mi = live * (row[:, MIMM_LO] | row[:, MIMM_HI] << 16)
    bv = live * (row[:, B_LO] | row[:, B_HI] << 16)
    r = live * (row[:, RES_LO] | row[:, RES_HI] << 16)
    if io:
        a, bv = np.where(ecw == 1, (waddr << 2) & M, a), np.where(ecw == 1, new, bv)
    ad = np.where(ecw == 1, (waddr << 2) & M, (a + mi) & M)
    k0 = live * (((a & 0xFFFF) + (mi & 0xFFFF)) >> 16)
    k1 = live * (((a >> 16) + (mi >> 16) + k0) >> 16)
    o0, o1, wl = ad & 1, (ad >> 1) & 1, (ad & 0xFFFF) >> 2
    byt = lambda v, k: (v >> (8 * k)) & 255
    store = sb + sh + sw + (_e if io else 0)
    r_ = t[:m]
    r_[:, G_SEL:G_SEL + 9] = sel
    r_[:, G_MULT], r_[:, G_OP], r_[:, G_TS] = 1, op, 3 * cyc + 1
    for c, v in ((G_A_LO, a & 0xFFFF), (G_A_HI, a >> 16), (G_MI_LO, mi & 0xFFFF), (G_MI_HI, mi >> 16), (G_B_LO, bv & 0xFFFF),
                 (G_B_HI, bv >> 16), (G_R_LO, r & 0xFFFF), (G_R_HI, r >> 16), (G_AD_LO, ad & 0xFFFF), (G_AD_HI, ad >> 16),
                 (G_K0, k0), (G_K1, k1), (G_WL, wl), (G_WL4, 4 * wl), (G_O0, o0), (G_O1, o1),
                 (G_S, (1 - o0) * (1 - o1)), (G_S + 1, o0 * (1 - o1)), (G_S + 2, (1 - o0) * o1), (G_S + 3, o0 * o1),
                 (G_W_LO, old & 0xFFFF), (G_W_HI, old >> 16), (G_N_LO, new & 0xFFFF), (G_N_HI, new >> 16)):
        r_[:, c] = v
    for k in range(4):
        r_[:, G_W + k], r_[:, G_N + k], r_[:, G_BB + k] = byt(old, k), byt(new, k), store * byt(bv, k)
    x = sum(r_[:, G_S + k] * r_[:, G_W + k] for k in range(4))
    h0, h1 = np.where(o1 == 1, byt(old, 2), byt(old, 0)), np.where(o1 == 1, byt(old, 3), byt(old, 1))
    top = lb * x + lh * h1
    r_[:, G_X], r_[:, G_H0], r_[:, G_H1], r_[:, G_TOP], r_[:, G_SG], r_[:, G_SL] = x, h0, h1, top, top >> 7, (2 * top) & 255
    for j, (u, v) in enumerate(BYTE_PAIRS):
        r_[:, G_AND + j] = r_[:, u] & r_[:, v]
    # the access before each one at its word: stable sort by address (the list is in timestamp order per word)
    order = np.argsort(waddr, kind="stable")
    ws, tss = waddr[order], r_[order, G_TS]
    first = np.ones(m, dtype=bool)
    first[1:] = ws[1:] != ws[:-1]
    pts = np.zeros(m, dtype=np.int64)
    pts[order] = np.where(first, 0, np.roll(tss, 1))
    dl = r_[:, G_TS] - pts - 1
    r_[:, G_PTS], r_[:, G_DL], r_[:, G_DH] = pts, dl & 0x3FFF, dl >> 14
    hist = np.zeros(1 << 16, dtype=np.int64)
    for c in RANGE_COLS:
        hist += np.bincount(r_[:, c], minlength=1 << 16)[: 1 << 16]
    byte_mult = np.zeros(3 << 16, dtype=np.int64)
    for u, v in BYTE_PAIRS:
        byte_mult += np.bincount(r_[:, u] << 8 | r_[:, v], minlength=3 << 16)
    shift_mult = np.bincount(256 + r_[:, G_TOP], minlength=rv32cf.SHIFT_USED).astype(np.int64)
    return t, hist, byte_mult, shift_mult


def memory_rows(mem, n_rows=None):
    """the boundary table of an access list -> (table (n_rows, MEMORY_COLS) int64, the RANGE16 counts it adds): one row
    per distinct word in ascending address order: INIT the old word of its first access, FINAL and FTS the new word and
    the timestamp of its last, SAME / GL / GH the limb-wise distance to the next row's address"""
    mem = _mem(mem)
    cyc, waddr, old, new = mem.T
    order = np.argsort(waddr, kind="stable")
    ws = waddr[order]
    first = np.ones(ws.size, dtype=bool)
    first[1:] = ws[1:] != ws[:-1]
    last = np.ones(ws.size, dtype=bool)
    last[:-1] = ws[:-1] != ws[1:]
    addr = ws[first]
    k = addr.size
    n_rows = 1 << log_rows(k) if n_rows is None else n_rows
    t = np.zeros((n_rows, MEMORY_COLS), dtype=np.int64)
    init, fin, fts = old[order][first], new[order][last], 3 * cyc[order][last] + 1
    wl, wh = addr & 0x3FFF, addr >> 14
    same, gl, gh = (np.zeros(k, dtype=np.int64) for _ in range(3))
    same[:-1] = wh[1:] == wh[:-1]
    gl[:-1] = same[:-1] * (wl[1:] - wl[:-1] - 1)
    gh[:-1] = (1 - same[:-1]) * (wh[1:] - wh[:-1] - 1)
    for c, v in ((B_WL, wl), (B_WH, wh), (B_I_LO, init & 0xFFFF), (B_I_HI, init >> 16), (B_F_LO, fin & 0xFFFF),
                 (B_F_HI, fin >> 16), (B_FTS, fts), (B_REAL, 1), (B_GL, gl), (B_GH, gh), (B_WL4, 4 * wl), (B_SAME, same),
                 (B_FINV, rv32im._inv(fts))):
        t[:k, c] = v
    hist = sum(np.bincount(t[:k, c], minlength=1 << 16) for c in MEMORY_RANGE)
    return t, hist.astype(np.int64)


def shard_tables(seg, data, init, final_expected, ecalls, image, mem, strict=True):
    """the nine canonical traces of one executed segment -> ([cpu, program, register, byte, range, shift, muldiv, memop,
    memory] canonical int64 arrays: the four lookup tables a multiplicity column each, cpu public values, register
    public values); the preprocessed matrices beside them are prep_tables(image).  ValueError for a segment whose memop
    or memory table would be taller than twice the cpu table"""
    tr, n, _pc_lo, _pc_hi = rv32.trace_of(seg, data)
    cpu, final, final_ts, hist, byte_mult, shift_mult, sends = cpu_rows(tr, n, seg.end_pc, init, ecalls, mem, strict)
    pubs = rv32.shard_publics(seg, init, final, final_expected)
    md, h2, b2, s2 = rv32im.muldiv_rows(sends, strict=strict)
    if _mem(mem).shape[0] > 2 * n:
        raise ValueError("segment %d: more accesses than twice the cpu table's rows" % seg.index)
    mo, h3, b3, s3 = memop_rows(cpu, mem)
    bd, h4 = memory_rows(mem)
    prog = rv32elf.program_mult(tr["pc"], tr["ins"], image)
    byt = np.zeros(1 << rv32.BYTE_LOG_ROWS, dtype=np.int64)
    byt[: 3 << 16] = byte_mult + b2 + b3
    sh = np.zeros(1 << rv32cf.SHIFT_LOG_ROWS, dtype=np.int64)
    sh[: rv32cf.SHIFT_USED] = shift_mult + s2 + s3
    return ([cpu, prog[:, None], rv32.register_rows(init, final, final_ts), byt[:, None], (hist + h2 + h3 + h4)[:, None],
             sh[:, None], md, mo, bd],) + pubs


def bus_balance(tables_canon, airs_):
    """rv32.bus_balance with a tuple read as padded with zeros (its trailing zeros dropped): what the permutation
    argument's random linear combination sees -> {bus: {tuple: sends - receives}}, the zero entries dropped"""
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
            for row, mm in zip(vals.tolist(), m[nz].tolist()):
                while row and row[-1] == 0:
                    row.pop()
                row = tuple(row)
                c[row] = (c[row] + sign * mm) % P
    return {bus: {k: v for k, v in c.items() if v % P} for bus, c in out.items()}
