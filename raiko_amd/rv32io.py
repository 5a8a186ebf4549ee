"""The io form of the rv32im-mem chip set (rv32mem.py, rv32link.py): ecalls bound to the run's input and exit code.
Ten tables per shard, rv32im-mem's nine in their order, then `io`; a key of its own (prep_width 48, as rv32im-mem's).

  the key      setup writes the program tuple of the word 0x00000073 with RS1 = 10, RS2 = 11, WREG = 10: the ecall row's
               A and B are then a0 and a1 through the register argument.  Decode is trusted to setup, as under rv32im-elf
  cpu          rv32im-mem's 141 columns (N_ECW and EC_OP are 0: the send to memop is gone), then T0_LO / T0_HI (the call
               number, x5), PT_TS / DT_LO / DT_HI (the access before it and the gap's limbs), R5 = 5 IS_SYS and T0Z (T0 is 0:
               HALT).  An ecall row reads x5 as a FOURTH register access at timestamp TSA -- rs1 is x10 there, so TSA is
               free for x5 -- and sends (TSA, T0, A, B, RES) on BUS_IO.  After a HALT row no row is active
  memop        rv32mem.memop_air(io=True): an ECW row obeys SW's constraints; its tuple comes from an io word row
  io           one HEAD row per ecall in cycle order (TS strictly increases, the gap in RANGE16), after a READ head one WORD
               row per word it transfers, then padding.  A head receives the cpu row's tuple; the call is one-hot HALT / READ
               / COMMIT with T0 = READ + 2 COMMIT.  HALT and COMMIT: RES = A.  READ: RES = GOT with GOT + F = cap (a1, 16-bit
               limbs, borrow KF) and POS + GOT + E = N_INPUT (14 / 16-bit limbs, carry C in {0, 1, 2}), every limb in
               RANGE16 so that no sum can wrap p, and F = 0 or E = 0 (the flags ZC / ZR): GOT = min(cap, N_INPUT - POS).
               REM counts the word rows still to follow (GOT on a READ head, one less on every word row, 0 elsewhere) and
               the next row is a word row exactly when REM is not 0 (Z the is-zero flag of REM, RINV its witness).  Word row
               k sends (16, TS, AD, 0, V, 0) on BUS_MEMOP with AD = A + 4 k (carries K, K1; word aligned: AD_LO = 4 AQ) and
               the stream tuple (POS_WL, POS_WH, V_LO, V_HI, 0, 0) on BUS_INPUT, which no table receives.  POS runs
               through the whole table, padding included: POS' = POS + WORD
  io publics   POS_START, POS_END, N_INPUT, HALTED, EXIT_LO, EXIT_HI, then 8 words no constraint reads: the digest of the
               shard's slice of the input as stream tuples -- rv32link's digest of the journal (pos, word, 0) at the io
               table's height

The verifier (rv32_sets.verify_rv32_shard(input_words=)) slices input_words[POS_START:POS_END], recomputes the digest
(reason 2 on a mismatch) and adds the receive claims on BUS_INPUT (rk_p3_verify_claims); check_io_chain binds the shards'
positions to each other and N_INPUT to the input's length, and returns the exit code and the words read.

The bytes RK_ECALL_COMMIT appends to the journal are bound by the commit form of this form (rv32commit.py, commit=True):
commit-word rows after a COMMIT head read the call's words through the memory argument and a commit log is a public
output.  Without it the journal is no part of the statement.  The FRI statements over an io proof are out of scope, as
for linked proofs.

`shard_tables` builds an io shard's ten traces in numpy: the yardstick for rk_exec_rv32io_shard_device."""
import numpy as np

from . import rv32, rv32cf, rv32elf, rv32im, rv32link, rv32mem
from .rv32 import ACTIVE, A_HI, A_LO, B_HI, B_LO, BUS_RANGE16, BUS_REGISTER, RES_HI, RES_LO, TSA
from .rv32mem import BUS_MEMOP, EC_OP, IS_SYS, N_ECW, PROGRAM_PREP, PROGRAM_TUPLE, bus_balance, program_air  # noqa: F401
BUS_IO, BUS_INPUT = 12, 13
ECALL_WORD = 0x00000073
HALT, READ, COMMIT = 0, 1, 2
IO_TABLE = 9                                       # the io table's index among a shard's ten
MAX_INPUT = 1 << 30
N_DIGEST = rv32link.N_DIGEST

# ---- cpu columns past rv32im-mem's 141
T0_LO = rv32mem.CPU_COLS
T0_HI, PT_TS, DT_LO, DT_HI, R5, T0Z = range(T0_LO + 1, T0_LO + 7)
CPU_COLS = T0_LO + 7
IO_TUPLE_CPU = [TSA, T0_LO, T0_HI, A_LO, A_HI, B_LO, B_HI, RES_LO, RES_HI]

# ---- io columns
(Q_HEAD, Q_WORD, Q_ACT, Q_HALT, Q_READ, Q_COMMIT, Q_TS, Q_T0, Q_ZERO, Q_OP16, Q_AD_LO, Q_AD_HI, Q_AQ, Q_K, Q_K1, Q_B_LO, Q_B_HI,
 Q_RES_LO, Q_RES_HI, Q_RH4, Q_REM, Q_Z, Q_RINV, Q_POS, Q_PL, Q_PL4, Q_PH, Q_NL, Q_NL4, Q_NH, Q_GL, Q_GL4, Q_GH, Q_EL, Q_EL4, Q_EH,
 Q_C, Q_FLO, Q_FHI, Q_KF, Q_ZC, Q_ZR, Q_V_LO, Q_V_HI, Q_GAP_L, Q_GAP_H, Q_HSEEN) = range(47)
IO_COLS = 47
IO_TUPLE = [Q_TS, Q_T0, Q_ZERO, Q_AD_LO, Q_AD_HI, Q_B_LO, Q_B_HI, Q_RES_LO, Q_RES_HI]
IO_MEMOP_TUPLE = [Q_OP16, Q_TS, Q_AD_LO, Q_AD_HI, Q_ZERO, Q_ZERO, Q_V_LO, Q_V_HI, Q_ZERO, Q_ZERO]
INPUT_TUPLE = [Q_PL, Q_PH, Q_V_LO, Q_V_HI, Q_ZERO, Q_ZERO]
IO_RANGE = [(c, Q_ACT) for c in (Q_AD_LO, Q_AD_HI, Q_AQ, Q_PL, Q_PL4, Q_PH)] + \
    [(c, Q_READ) for c in (Q_RH4, Q_NL, Q_NL4, Q_NH, Q_GL, Q_GL4, Q_GH, Q_EL, Q_EL4, Q_EH, Q_FLO, Q_FHI)] + \
    [(Q_GAP_L, Q_HEAD), (Q_GAP_H, Q_HEAD), (Q_V_LO, Q_WORD), (Q_V_HI, Q_WORD)]
# ---- io public values
PUB_POS_START, PUB_POS_END, PUB_N_INPUT, PUB_HALTED, PUB_EXIT_LO, PUB_EXIT_HI, PUB_DIGEST = range(7)
N_PUBLIC_IO = PUB_DIGEST + N_DIGEST
MIN_LOG = 1


# ------------------------------------------------------------------------------------------------ the AIRs
def cpu_air(ext_w=None):
    """-> the cpu Air of the io form: rv32im's body over rv32im-mem's program tuple, the send of loads and stores to
    memop, the x5 access of an ecall row and its send to the io table"""
    from . import p3
    b = p3.AirBuilder(CPU_COLS, rv32.N_PUBLIC_CPU, p3.EXT_W if ext_w is None else ext_w)
    names = rv32im.cpu_constraints(b, PROGRAM_TUPLE)
    named = rv32im._namer(b, names)
    L = b.local
    M = rv32mem
    b.send(BUS_MEMOP, [M.MEM_OP, TSA, A_LO, A_HI, M.MIMM_LO, M.MIMM_HI, B_LO, B_HI, RES_LO, RES_HI], mult=M.M_MEM, mult_is_const=False)
    b.receive(BUS_REGISTER, [R5, T0_LO, T0_HI, PT_TS], mult=IS_SYS, mult_is_const=False)
    b.send(BUS_REGISTER, [R5, T0_LO, T0_HI, TSA], mult=IS_SYS, mult_is_const=False)
    b.send(BUS_IO, IO_TUPLE_CPU, mult=IS_SYS, mult_is_const=False)
    b.send(BUS_RANGE16, [DT_LO], mult=IS_SYS, mult_is_const=False)
    b.send(BUS_RANGE16, [DT_HI], mult=IS_SYS, mult_is_const=False)
    sys_, t0 = L(IS_SYS), L(T0_LO)
    named("m_mem", L(M.M_MEM) - L(M.IS_LOAD) * L(rv32.WR) - L(M.IS_STORE) * L(ACTIVE))
    named("n_ecw", L(N_ECW))
    named("ec_op", L(EC_OP))
    named("sys padding", (1 - L(ACTIVE)) * sys_)           # IS_SYS is looked up on active rows only
    named("r5", L(R5) - sys_ * 5)
    named("t0 ts", sys_ * (L(TSA) - L(PT_TS) - 1 - L(DT_LO) - L(DT_HI) * 16384))
    # T0Z = 1 exactly on a HALT row (the io table bounds T0 to {0, 1, 2}); after it no row is active
    named("t0z", sys_ * (L(T0Z) * 2 - (1 - t0) * (2 - t0)))
    named("t0z sys", (1 - sys_) * L(T0Z))
    named("halt ends", b.is_transition() * L(T0Z) * b.next(ACTIVE))
    air = b.build()
    air.constraint_names = names
    return air


def io_air(ext_w=None):
    """-> the io Air; its `constraint_names` maps the name of each constraint to its index"""
    from . import p3
    b = p3.AirBuilder(IO_COLS, N_PUBLIC_IO, p3.EXT_W if ext_w is None else ext_w)
    L, N = b.local, b.next
    names = {}
    named = rv32im._namer(b, names)
    b.receive(BUS_IO, IO_TUPLE, mult=Q_HEAD, mult_is_const=False)
    b.send(BUS_MEMOP, IO_MEMOP_TUPLE, mult=Q_WORD, mult_is_const=False)
    b.send(BUS_INPUT, INPUT_TUPLE, mult=Q_WORD, mult_is_const=False)          # received by the verifier
    for c, m in IO_RANGE:
        b.send(BUS_RANGE16, [c], mult=m, mult_is_const=False)
    head, word, act, halt, read, commit = (L(c) for c in (Q_HEAD, Q_WORD, Q_ACT, Q_HALT, Q_READ, Q_COMMIT))
    tr = b.is_transition()
    for tag, c in (("head", Q_HEAD), ("word", Q_WORD), ("act", Q_ACT), ("halt", Q_HALT), ("read", Q_READ), ("commit", Q_COMMIT),
                   ("k", Q_K), ("k1", Q_K1), ("z", Q_Z), ("kf", Q_KF), ("zc", Q_ZC), ("zr", Q_ZR), ("hseen", Q_HSEEN)):
        named("bool " + tag, L(c) * (L(c) - 1))
    named("act", act - head - word)
    named("call", head - halt - read - commit)                 # one-hot: no other call has a row
    named("t0", L(Q_T0) - read - commit * 2)
    named("zero", L(Q_ZERO))
    named("op16", L(Q_OP16) - word * rv32mem.EC_CODE)
    named("padding", tr * (1 - act) * N(Q_ACT))
    named("first is no word", b.is_first_row() * word)
    # HALT and COMMIT leave a0; READ leaves GOT
    keep = halt + commit
    named("keep lo", keep * (L(Q_RES_LO) - L(Q_AD_LO)))
    named("keep hi", keep * (L(Q_RES_HI) - L(Q_AD_HI)))
    got = L(Q_GL) + L(Q_GH) * 16384
    named("got", read * (L(Q_RES_LO) + L(Q_RES_HI) * 65536 - got))          # RES_HI < 2^14 (RH4): both sides < 2^30
    for tag, c4, c in (("rh4", Q_RH4, Q_RES_HI), ("gl4", Q_GL4, Q_GL), ("pl4", Q_PL4, Q_PL), ("nl4", Q_NL4, Q_NL), ("el4", Q_EL4, Q_EL)):
        named(tag, L(c4) - L(c) * 4)
    # GOT + F = cap, limb by limb
    named("cap lo", read * (L(Q_RES_LO) + L(Q_FLO) - L(Q_B_LO) - L(Q_KF) * 65536))
    named("cap hi", read * (L(Q_RES_HI) + L(Q_FHI) + L(Q_KF) - L(Q_B_HI)))
    # POS + GOT + E = N_INPUT, limb by limb (14 / 16 bits); the carry of three 14-bit limbs is 0, 1 or 2
    c = L(Q_C)
    named("carry", c * (c - 1) * (c - 2))
    named("left lo", read * (L(Q_PL) + L(Q_GL) + L(Q_EL) - L(Q_NL) - c * 16384))
    named("left hi", read * (L(Q_PH) + L(Q_GH) + L(Q_EH) + c - L(Q_NH)))
    named("n_input", read * (L(Q_NL) + L(Q_NH) * 16384 - b.public(PUB_N_INPUT)))
    named("zc", L(Q_ZC) * (L(Q_FLO) + L(Q_FHI)))
    named("zr", L(Q_ZR) * (L(Q_EL) + L(Q_EH)))
    named("min", read * (1 - L(Q_ZC)) * (1 - L(Q_ZR)))
    # exactly GOT word rows follow a READ head
    rem, z = L(Q_REM), L(Q_Z)
    named("rem read", read * (rem - got))
    named("rem keep", keep * rem)
    named("rem padding", (1 - act) * rem)
    named("z", z * rem)
    named("rinv", 1 - z - rem * L(Q_RINV))
    named("word follows", tr * (N(Q_WORD) - 1 + z))
    named("rem ends", b.is_last_row() * (1 - z))
    named("rem counts", tr * N(Q_WORD) * (N(Q_REM) - rem + 1))
    # a word row carries its head's TS; its address is A + 4 k
    named("word ts", tr * N(Q_WORD) * (N(Q_TS) - L(Q_TS)))
    named("first lo", tr * N(Q_WORD) * head * (N(Q_AD_LO) - L(Q_AD_LO)))
    named("first hi", tr * N(Q_WORD) * head * (N(Q_AD_HI) - L(Q_AD_HI)))
    named("next lo", tr * N(Q_WORD) * word * (N(Q_AD_LO) + N(Q_K) * 65536 - L(Q_AD_LO) - 4))
    named("next hi", tr * N(Q_WORD) * word * (N(Q_AD_HI) + N(Q_K1) * 65536 - L(Q_AD_HI) - N(Q_K)))
    named("aligned", (read + word) * (L(Q_AD_LO) - L(Q_AQ) * 4))
    # heads in cycle order
    named("order", tr * N(Q_HEAD) * (N(Q_TS) - L(Q_TS) - 1 - N(Q_GAP_L) - N(Q_GAP_H) * 16384))
    # the stream position
    named("pos", tr * (N(Q_POS) - L(Q_POS) - word))
    named("pos limbs", act * (L(Q_POS) - L(Q_PL) - L(Q_PH) * 16384))
    named("pos start", b.is_first_row() * (L(Q_POS) - b.public(PUB_POS_START)))
    named("pos end", b.is_last_row() * (L(Q_POS) + word - b.public(PUB_POS_END)))
    # HALT
    named("hseen first", b.is_first_row() * (L(Q_HSEEN) - halt))
    named("hseen", tr * (N(Q_HSEEN) - L(Q_HSEEN) - N(Q_HALT)))
    named("halted", b.is_last_row() * (L(Q_HSEEN) - b.public(PUB_HALTED)))
    named("exit lo", halt * (L(Q_AD_LO) - b.public(PUB_EXIT_LO)))
    named("exit hi", halt * (L(Q_AD_HI) - b.public(PUB_EXIT_HI)))
    air = b.build()
    air.constraint_names = names
    return air


def airs(ext_w=None, link=False):
    """-> (cpu, program, register, byte, range, shift, muldiv, memop, memory, io): the AIRs of one io shard.  link: the
    memory AIR is rv32link's"""
    return (cpu_air(ext_w), program_air(ext_w), rv32.register_air(ext_w), rv32elf.byte_air(ext_w), rv32elf.range_air(ext_w),
            rv32elf.shift_air(ext_w), rv32im.muldiv_air(ext_w), rv32mem.memop_air(ext_w, io=True),
            rv32link.memory_air(ext_w) if link else rv32mem.memory_air(ext_w), io_air(ext_w))


# ------------------------------------------------------------------------------------------------ the key
def prep_tables(image):
    """rv32mem.prep_tables with the ecall word's tuple reading a0 and a1: RS1 = 10, RS2 = 11 (WREG is 10 already)"""
    prog, byt, rng, sh = rv32mem.prep_tables(image)
    ecall = (prog[:, 2] | prog[:, 3] << 16) == ECALL_WORD
    prog[ecall, 4], prog[ecall, 5] = 10, 11
    return prog, byt, rng, sh


def preps_of(image):
    """prep_tables in table order: None for the tables without preprocessed columns"""
    prog, byt, rng, sh = prep_tables(image)
    return [None, prog, None, byt, rng, sh, None, None, None, None]


# ------------------------------------------------------------------------------------------------ the stream
def stream_journal(pos_start, words):
    """a slice of the input as the journal rv32link's digest and claims take: (k, 3) uint32 -- position, word, 0"""
    w = np.asarray(words, dtype=np.int64).reshape(-1) & 0xFFFFFFFF
    return np.stack([pos_start + np.arange(w.size, dtype=np.int64), w, np.zeros(w.size, dtype=np.int64)], axis=1).astype(np.uint32)


def stream_root(pos_start, words, log_rows, params=None):
    """the digest of a slice of the input at io-table height 2^log_rows -> 8 Montgomery words (rk_rv32mem_journal_root)"""
    return rv32link.journal_root(stream_journal(pos_start, words), log_rows, params)


def claims_of(pos_start, words):
    """what a verifier adds for a shard's slice of the input: p3.verify(..., claims=claims_of(POS_START, slice))"""
    from . import p3
    return [(BUS_INPUT, -1, p3.to_mont(rv32link.journal_tuples(stream_journal(pos_start, words))))]


def publics_of(public_mont):
    """the io table's public values (14 Montgomery words) -> dict: pos_start, pos_end, n_input, halted, exit, digest (8
    Montgomery words), and `limbs` -- whether EXIT's limbs are 16-bit values"""
    from . import p3
    pv = np.asarray(public_mont, dtype=np.uint32).reshape(-1)
    if pv.size != N_PUBLIC_IO:
        raise ValueError("the io table carries %d public values" % N_PUBLIC_IO)
    c = p3.from_mont(pv[:PUB_DIGEST]).astype(np.int64)
    return dict(pos_start=int(c[PUB_POS_START]), pos_end=int(c[PUB_POS_END]), n_input=int(c[PUB_N_INPUT]), halted=int(c[PUB_HALTED]),
                exit=int(c[PUB_EXIT_LO] | c[PUB_EXIT_HI] << 16), limbs=bool(c[PUB_EXIT_LO] < 1 << 16 and c[PUB_EXIT_HI] < 1 << 16),
                digest=pv[PUB_DIGEST:].copy())


def slice_of(pub, input_words):
    """the shard's slice of the verifier's input, or None when the public values do not fit it: N_INPUT is not its length
    (or 2^30 words and more), POS_START <= POS_END <= N_INPUT fails, HALTED is no bit, EXIT no 32-bit word or set without
    HALTED"""
    n = len(input_words)
    if n >= MAX_INPUT or pub["n_input"] != n or not 0 <= pub["pos_start"] <= pub["pos_end"] <= n:
        return None
    if pub["halted"] not in (0, 1) or not pub["limbs"] or (pub["exit"] and not pub["halted"]):
        return None
    return np.asarray(input_words, dtype=np.int64)[pub["pos_start"]:pub["pos_end"]] & 0xFFFFFFFF


def check_io_chain(publics, input_words):
    """the chaining of an io run over its shards' io public values (publics: publics_of per shard): shard 0 reads from
    position 0, every shard from where the one before stopped, N_INPUT is len(input_words) on every shard, HALTED is set
    on the last shard at most.  Raises ValueError naming the shard -> (exit code: None for a run that has not halted,
    input words read)"""
    n, pos = len(input_words), 0
    if n >= MAX_INPUT:
        raise ValueError("an input of 2^30 words or more")
    for k, pub in enumerate(publics):
        if pub["n_input"] != n:
            raise ValueError("shard %d: N_INPUT is %d, the input has %d words" % (k, pub["n_input"], n))
        if pub["pos_start"] != pos:
            raise ValueError("shard %d: reads the input from word %d, the shards before stopped at %d" % (k, pub["pos_start"], pos))
        if not pos <= pub["pos_end"] <= n:
            raise ValueError("shard %d: stops reading at word %d of %d" % (k, pub["pos_end"], n))
        if pub["halted"] not in (0, 1) or (pub["halted"] and k + 1 != len(publics)):
            raise ValueError("shard %d: halts before the last shard" % k)
        if not pub["limbs"] or (pub["exit"] and not pub["halted"]):
            raise ValueError("shard %d: an exit code without a halt" % k)
        pos = pub["pos_end"]
    last = publics[-1] if publics else None
    return (last["exit"] if last is not None and last["halted"] else None), pos


# ------------------------------------------------------------------------------------------------ numpy witness
def _args(args):
    return np.asarray(args, dtype=np.int64).reshape(-1, 5)


def io_trace(tr, args):
    """the trace as the io key decodes it: an ecall row is `ecall a0, a1` -- its word reads x10 and x11 and its A and B
    are the side list's a0 and a1 (TraceRow.a / .b stay 0 in the executor: other chip sets read them).  args: (k, 5):
    cycle, t0, a0 before, a1, input position before (rk_exec_ecall_args).  ValueError for a side list that is not the
    trace's ecall rows"""
    args = _args(args)
    ins = np.asarray(tr["ins"], dtype=np.int64)
    want = np.nonzero(ins == ECALL_WORD)[0]
    if args.shape[0] != want.size or not np.array_equal(args[:, 0], want):
        raise ValueError("ecall side list does not match the trace")
    out = {k: np.asarray(v, dtype=np.int64).copy() for k, v in tr.items()}
    out["ins"][want] = ECALL_WORD | 10 << 15 | 11 << 20
    out["a"][want], out["b"][want] = args[:, 2], args[:, 3]
    return out


def cpu_rows(tr, n, end_pc, init, ecalls, mem, args, strict=True):
    """rv32mem.cpu_rows over io_trace with the seven columns appended and the x5 access of every ecall row threaded into
    the register argument: the access after it at x5 (or the register table's final timestamp) follows it -> rv32mem
    .cpu_rows's tuple.  ValueError when the side list's t0 is not what x5 holds"""
    args = _args(args)
    base, final, final_ts, hist, byte_mult, shift_mult, sends = rv32mem.cpu_rows(io_trace(tr, args), n, end_pc, init, ecalls, mem, strict)
    cyc = tr["pc"].size
    t = np.zeros((n, CPU_COLS), dtype=np.int64)
    t[:, :rv32mem.CPU_COLS] = base
    ec = args[:, 0]
    t[ec, rv32.INS_LO], t[ec, rv32.INS_HI] = ECALL_WORD, 0
    t[:, N_ECW] = 0
    t[:, EC_OP] = 0
    # every access of x5, in timestamp order: kind 0 / 1 / 2 = rs1 / rs2 / rd of a row, 3 = an ecall row's
    act = t[:cyc]
    rows = np.arange(cyc, dtype=np.int64)
    kinds = [(rows[act[:, rv32.RS1] == 5], 0), (rows[act[:, rv32.RS2] == 5], 1),
             (rows[(act[:, rv32.WR] == 1) & (act[:, rv32.WREG] == 5)], 2), (ec, 3)]
    row = np.concatenate([r for r, _k in kinds])
    kind = np.concatenate([np.full(r.size, k, dtype=np.int64) for r, k in kinds])
    ts = 3 * row + 1 + np.where(kind == 3, 0, kind)
    order = np.argsort(ts, kind="stable")
    row, kind, ts = row[order], kind[order], ts[order]
    t0 = dict(zip(ec.tolist(), args[:, 1].tolist()))
    val_col = {0: (A_LO, A_HI), 1: (B_LO, B_HI), 2: (RES_LO, RES_HI)}
    prev_col = {0: (rv32.PA_TS, rv32.DA_LO, rv32.DA_HI), 1: (rv32.PB_TS, rv32.DB_LO, rv32.DB_HI), 2: (rv32.PW_TS, rv32.DW_LO, rv32.DW_HI)}
    x5, x5_ts = int(init[5]), 0
    for j in range(row.size):
        r, k, at = int(row[j]), int(kind[j]), int(ts[j])
        if k == 3:
            if t0[r] != x5:
                raise ValueError("ecall side list does not match the trace: t0 is not what x5 holds")
            gap = at - x5_ts - 1
            t[r, T0_LO], t[r, T0_HI], t[r, PT_TS], t[r, DT_LO], t[r, DT_HI] = x5 & 0xFFFF, x5 >> 16, x5_ts, gap & 0x3FFF, gap >> 14
            hist[gap & 0x3FFF] += 1
            hist[gap >> 14] += 1
        else:
            if j and kind[j - 1] == 3:                     # its predecessor is the ecall row's read, not what rv32 resolved
                pc_, lo_, hi_ = prev_col[k]
                hist[t[r, lo_]] -= 1
                hist[t[r, hi_]] -= 1
                gap = at - x5_ts - 1
                t[r, pc_], t[r, lo_], t[r, hi_] = x5_ts, gap & 0x3FFF, gap >> 14
                hist[gap & 0x3FFF] += 1
                hist[gap >> 14] += 1
            lo_, hi_ = val_col[k]
            x5 = int(t[r, lo_] | t[r, hi_] << 16)
        x5_ts = at
    if row.size and kind[-1] == 3:
        final_ts = final_ts.copy()
        final_ts[5] = x5_ts
    t[ec, R5] = 5
    t[ec, T0Z] = (args[:, 1] == HALT).astype(np.int64)
    return t, final, final_ts, hist, byte_mult, shift_mult, sends


def log_rows(count):
    lg = MIN_LOG
    while (1 << lg) < count:
        lg += 1
    return lg


def io_rows(args, ecalls, mem, n_input, pos_start=None, n_rows=None):
    """the io table of a shard's ecalls -> (table (n_rows, IO_COLS) int64, the RANGE16 counts it adds, its six leading
    public values, canonical).  args: the side list (k, 5); ecalls: (cycle, a0 after) of the same rows; mem: the access
    list, whose entries at a READ's cycle are the words it stored; n_input: the length of the run's input.  pos_start:
    where the shard's stream starts when it has no ecall (else the first ecall's position).  n_rows None: 2^log_rows(heads
    + words).  ValueError for lists that do not agree, a READ that stores other than min(cap, left) words or an input of
    2^30 words and more"""
    args, mem = _args(args), rv32mem._mem(mem)
    ec = np.asarray(ecalls, dtype=np.int64).reshape(-1, 2)
    if n_input >= MAX_INPUT:
        raise ValueError("an input of 2^30 words or more")
    if ec.shape[0] != args.shape[0] or not np.array_equal(ec[:, 0], args[:, 0]):
        raise ValueError("ecall side list does not match the trace")
    M = 0xFFFFFFFF
    rows = []
    pos = int(args[0, 4]) if args.shape[0] else int(pos_start or 0)
    start = pos
    halted, exit_code, last_ts = 0, 0, None
    for (cycle, t0, a0, a1, p0), (_c, res) in zip(args.tolist(), ec.tolist()):
        if t0 not in (HALT, READ, COMMIT):
            raise ValueError("an ecall that is none of HALT, READ, COMMIT")
        if p0 != pos:
            raise ValueError("the side list's input positions do not follow the words read")
        ts = 3 * cycle + 1
        r = np.zeros(IO_COLS, dtype=np.int64)
        r[Q_HEAD] = r[Q_ACT] = 1
        r[Q_HALT + t0] = 1
        r[Q_TS], r[Q_T0] = ts, t0
        r[Q_AD_LO], r[Q_AD_HI], r[Q_B_LO], r[Q_B_HI], r[Q_RES_LO], r[Q_RES_HI] = a0 & 0xFFFF, a0 >> 16, a1 & 0xFFFF, a1 >> 16, res & 0xFFFF, res >> 16
        r[Q_POS], r[Q_PL], r[Q_PH] = pos, pos & 0x3FFF, pos >> 14
        gap = 0 if last_ts is None else ts - last_ts - 1
        r[Q_GAP_L], r[Q_GAP_H] = gap & 0x3FFF, gap >> 14
        last_ts = ts
        words = mem[mem[:, 0] == cycle] if t0 == READ else mem[:0]
        if t0 == READ:
            got, left = words.shape[0], n_input - pos
            if got != min(a1, left) or res != got or a0 & 3:
                raise ValueError("a READ that does not store min(capacity, words left) words at an aligned address")
            f, e = a1 - got, left - got
            r[Q_AQ] = (a0 & 0xFFFF) >> 2
            r[Q_REM] = got
            r[Q_NL], r[Q_NH] = n_input & 0x3FFF, n_input >> 14
            r[Q_GL], r[Q_GH] = got & 0x3FFF, got >> 14
            r[Q_EL], r[Q_EH] = e & 0x3FFF, e >> 14
            r[Q_C] = ((pos & 0x3FFF) + (got & 0x3FFF) + (e & 0x3FFF)) >> 14
            r[Q_FLO], r[Q_FHI] = f & 0xFFFF, f >> 16
            r[Q_KF] = ((got & 0xFFFF) + (f & 0xFFFF)) >> 16
            r[Q_ZC], r[Q_ZR] = int(f == 0), int(e == 0)
        elif res != a0:
            raise ValueError("a HALT or COMMIT that changes a0")
        if t0 == HALT:
            halted, exit_code = 1, a0
        rows.append(r)
        ad = a0
        for k, (_cy, waddr, _old, new) in enumerate(words.tolist()):
            if waddr != ((a0 + 4 * k) & M) >> 2:
                raise ValueError("a READ whose words are not stored in ascending order from its destination")
            w = np.zeros(IO_COLS, dtype=np.int64)
            nad = (a0 + 4 * k) & M
            w[Q_WORD] = w[Q_ACT] = 1
            w[Q_TS], w[Q_OP16] = ts, rv32mem.EC_CODE
            w[Q_AD_LO], w[Q_AD_HI], w[Q_AQ] = nad & 0xFFFF, nad >> 16, (nad & 0xFFFF) >> 2
            if k:
                w[Q_K] = ((ad & 0xFFFF) + 4) >> 16
                w[Q_K1] = ((ad >> 16) + w[Q_K]) >> 16
            ad = nad
            w[Q_REM] = len(words) - 1 - k
            w[Q_POS], w[Q_PL], w[Q_PH] = pos, pos & 0x3FFF, pos >> 14
            w[Q_V_LO], w[Q_V_HI] = new & 0xFFFF, new >> 16
            pos += 1
            rows.append(w)
    n_rows = 1 << log_rows(len(rows)) if n_rows is None else n_rows
    t = np.zeros((n_rows, IO_COLS), dtype=np.int64)
    if rows:
        t[:len(rows)] = np.stack(rows)
    t[len(rows):, Q_POS] = pos
    t[:, Q_PL4], t[:, Q_NL4], t[:, Q_GL4], t[:, Q_EL4] = 4 * t[:, Q_PL], 4 * t[:, Q_NL], 4 * t[:, Q_GL], 4 * t[:, Q_EL]
    t[:, Q_RH4] = 4 * t[:, Q_RES_HI]
    t[:, Q_Z] = t[:, Q_REM] == 0
    t[:, Q_RINV] = rv32im._inv(t[:, Q_REM])
    t[:, Q_HSEEN] = np.cumsum(t[:, Q_HALT])
    hist = np.zeros(1 << 16, dtype=np.int64)
    for c, m in IO_RANGE:
        hist += np.bincount(t[t[:, m] == 1, c], minlength=1 << 16)[: 1 << 16]
    pubs = np.array([start, pos, n_input, halted, exit_code & 0xFFFF, exit_code >> 16], dtype=np.int64)
    return t, hist, pubs


def io_publics(pubs, table_rows, stream_words, params=None):
    """the io table's 14 public values as the prover commits them (Montgomery words): the six leading ones and the
    digest of the shard's slice of the input at the table's height"""
    from . import p3
    digest = stream_root(int(pubs[PUB_POS_START]), stream_words, table_rows.bit_length() - 1, params)
    return np.concatenate([p3.to_mont(pubs), digest])


def shard_tables(seg, data, init, final_expected, ecalls, image, mem, args, n_input, pos_start=None, strict=True, params=None,
                 link=False):
    """rv32mem.shard_tables of an io shard -> (the ten canonical traces, cpu public values, register public values, the
    memory table's public values -- the journal's digest with link, else () --, the io table's public values: 14
    Montgomery words).  The preprocessed matrices beside them are prep_tables(image)"""
    tr, n, _pc_lo, _pc_hi = rv32.trace_of(seg, data)
    cpu, final, final_ts, hist, byte_mult, shift_mult, sends = cpu_rows(tr, n, seg.end_pc, init, ecalls, mem, args, strict)
    pubs = rv32.shard_publics(seg, init, final, final_expected)
    md, h2, b2, s2 = rv32im.muldiv_rows(sends, strict=strict)
    if rv32mem._mem(mem).shape[0] > 2 * n:
        raise ValueError("segment %d: more accesses than twice the cpu table's rows" % seg.index)
    mo, h3, b3, s3 = rv32mem.memop_rows(cpu, mem, io=True)
    bd, h4 = rv32mem.memory_rows(mem)
    io, h5, io_pubs = io_rows(args, ecalls, mem, n_input, pos_start)
    if io.shape[0] > 2 * n:
        raise ValueError("segment %d: more io rows than twice the cpu table's rows" % seg.index)
    prog = rv32elf.program_mult(tr["pc"], tr["ins"], image)
    byt = np.zeros(1 << rv32.BYTE_LOG_ROWS, dtype=np.int64)
    byt[: 3 << 16] = byte_mult + b2 + b3
    sh = np.zeros(1 << rv32cf.SHIFT_LOG_ROWS, dtype=np.int64)
    sh[: rv32cf.SHIFT_USED] = shift_mult + s2 + s3
    words = io[io[:, Q_WORD] == 1]
    stream = words[:, Q_V_LO] | words[:, Q_V_HI] << 16
    digest = rv32link.journal_root(rv32link.journal_of_table(bd), bd.shape[0].bit_length() - 1, params) if link else ()
    return ([cpu, prog[:, None], rv32.register_rows(init, final, final_ts), byt[:, None], (hist + h2 + h3 + h4 + h5)[:, None],
             sh[:, None], md, mo, bd, io],) + pubs + (digest, io_publics(io_pubs, io.shape[0], stream, params))
