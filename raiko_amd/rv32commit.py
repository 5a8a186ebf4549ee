"""The commit form of the io form of the rv32im-mem chip set (rv32io.py, commit=True): the bytes RK_ECALL_COMMIT appends
to the journal are read through the memory argument and the journal is a public output.  Ten tables per shard, the io
form's in their order under the io form's key (the decode does not differ); a verifier tells the form apart by the io
table's 24 public values.  cpu, program, register, byte, range, shift, muldiv and memory are rv32io's.

  memop        rv32mem.memop_air(io=True, commit=True): 65 columns, the last the selector of a tenth row kind, ECR (op
               17): it obeys LW's constraints -- word aligned, R the word before, the word unchanged -- so R is the word the
               shard's memory history holds at TS.  Its tuple comes from a commit-word row of the io table
  io           rv32io's 47 columns and constraints, then CW, S, S0, S1, CNT, C0, C1, T0B, T1B, BH7, RML, RMH, RMH7, JPOS,
               JL, JL4, JH (64 columns).  After a COMMIT head with a1 != 0 come its commit-word rows (CW = 1), one per word
               the call reads: NCW = ((a0 & 3) + a1 + 3) >> 2 of them.  Row k carries the head's TS, reads the word at
               AD = (a0 & ~3) + 4 k (the carries K, K1 of READ's word rows; AD_LO = 4 AQ) and sends (17, TS, AD, 0, 0, V) on
               BUS_MEMOP: V is memory's word.  S = S0 + 2 S1 and CNT = 1 + C0 + 2 C1 (bits; CNT = 0 off commit-word rows)
               say which bytes go to the journal: bytes S .. S + CNT - 1 of V, little endian.  S + CNT + T = 4 with the
               slack T = T0B + 2 T1B: CNT >= 1 and S + CNT <= 4.  On the first row AD_LO + S is the head's AD_LO: with AD_LO
               aligned and both in RANGE16 that is S = a0 & 3; on every later row S = 0.  REM, Z and RINV count bytes here:
               REM = a1 on a COMMIT head (0 on HALT), REM' = REM - CNT' into a commit-word row, and the next row is a
               commit-word row exactly when REM is not 0 -- so the CNT of a call sum to a1 -- and T = 0 unless Z: every row
               but the call's last is filled to the word's end.  These force the rows of a call uniquely from (a0, a1).
               JPOS, the byte offset into the run's journal, runs through the whole table: JPOS' = JPOS + CNT.  A
               commit-word row sends (JL, JH, V_LO, V_HI, S, CNT) on BUS_COMMIT = 14, which no table receives
  io publics   rv32io's 14, then JPOS_START, JPOS_END and 8 words no constraint reads: the digest of the shard's commit
               log -- rv32link's digest of the journal (jpos, word, S | CNT << 16) at the io table's height

No sum wraps p = 2^31 - 2^27 + 1.  a1 < 2^25: BH7 = 128 B_HI is in RANGE16 on a COMMIT head and B's limbs are a register's.
On a commit-word row REM = RML + 2^16 RMH with RML, RMH and RMH7 = 128 RMH in RANGE16, so REM < 2^25 as an integer: from
REM < 2^25 before and CNT <= 4, REM - CNT lies in (-4, 2^25) and a negative one, p - d, has no such limbs -- the countdown
reaches 0 exactly and cannot step over it.  (The executor's cap of 16 MiB on the journal binds no prover; 2^25 is the
circuit's.)  JPOS = JL + 2^14 JH with JL, 4 JL and JH in RANGE16 on every commit-word row: below 2^30, and the verifier
walks the log's positions as integers from JPOS_START < 2^30.  S, CNT and T are sums of bits.  V is not sent to RANGE16:
the memop row that answers it builds the word from looked-up bytes.

The verifier (rv32_sets.verify_rv32_shard(commit_log=)) is handed the shard's commit log as the link's verifier is handed
the memory journal: it checks the log's shape (log_bytes: positions consecutive from JPOS_START to JPOS_END, 1 <= CNT,
S + CNT <= 4), recomputes the digest (reason 2 on a mismatch), adds the receive claims on BUS_COMMIT and cuts bytes
S .. S + CNT - 1 out of every word: the shard's slice of the journal.  check_commit_chain binds the shards' positions to
each other.  The log reveals the bytes of the first and last word of a COMMIT that the call does not select: nothing
here is zero-knowledge.  The verifier's work is linear in the journal.

STILL FREE: nothing of an ecall.  The FRI statements over a commit proof are out of scope, as for linked and io proofs.

`shard_tables` builds a commit shard's ten traces in numpy: the yardstick for rk_exec_rv32commit_shard_device."""
import numpy as np

from . import rv32, rv32cf, rv32elf, rv32im, rv32io, rv32link, rv32mem
from .rv32 import BUS_RANGE16
from .rv32io import (BUS_INPUT, BUS_IO, COMMIT, HALT, INPUT_TUPLE, IO_MEMOP_TUPLE, IO_TABLE, IO_TUPLE, PUB_EXIT_HI, PUB_EXIT_LO,  # noqa: F401
                     PUB_HALTED, PUB_N_INPUT, PUB_POS_END, PUB_POS_START, Q_ACT, Q_AD_HI, Q_AD_LO, Q_AQ, Q_B_HI, Q_B_LO, Q_C,
                     Q_COMMIT, Q_EH, Q_EL, Q_EL4, Q_FHI, Q_FLO, Q_GAP_H, Q_GAP_L, Q_GH, Q_GL, Q_GL4, Q_HALT, Q_HEAD, Q_HSEEN, Q_K,
                     Q_K1, Q_KF, Q_NH, Q_NL, Q_NL4, Q_OP16, Q_PH, Q_PL, Q_PL4, Q_POS, Q_READ, Q_REM, Q_RES_HI, Q_RES_LO, Q_RH4,
                     Q_RINV, Q_T0, Q_TS, Q_V_HI, Q_V_LO, Q_WORD, Q_Z, Q_ZC, Q_ZERO, Q_ZR, READ, bus_balance, cpu_air, preps_of,
                     prep_tables, program_air)
from .rv32mem import BUS_MEMOP, G_ECR, MEMOP_COLS_COMMIT

BUS_COMMIT = 14
ECR_CODE = rv32mem.ECR_CODE
MAX_JOURNAL = 1 << 30
MAX_COMMIT = 1 << 25                               # a1 of one COMMIT, bounded in circuit
N_DIGEST = rv32link.N_DIGEST

# ---- io columns past rv32io's 47
(Q_CW, Q_S, Q_S0, Q_S1, Q_CNT, Q_C0, Q_C1, Q_T0B, Q_T1B, Q_BH7, Q_RML, Q_RMH, Q_RMH7, Q_JPOS, Q_JL, Q_JL4,
 Q_JH) = range(rv32io.IO_COLS, rv32io.IO_COLS + 17)
IO_COLS = rv32io.IO_COLS + 17
IO_MEMOP_TUPLE_CW = [Q_OP16, Q_TS, Q_AD_LO, Q_AD_HI, Q_ZERO, Q_ZERO, Q_ZERO, Q_ZERO, Q_V_LO, Q_V_HI]
COMMIT_TUPLE = [Q_JL, Q_JH, Q_V_LO, Q_V_HI, Q_S, Q_CNT]
IO_RANGE = rv32io.IO_RANGE + [(Q_BH7, Q_COMMIT)] + [(c, Q_CW) for c in (Q_RML, Q_RMH, Q_RMH7, Q_JL, Q_JL4, Q_JH)]
# ---- io public values past rv32io's 14
PUB_JPOS_START = rv32io.N_PUBLIC_IO
PUB_JPOS_END, PUB_COMMIT_DIGEST = PUB_JPOS_START + 1, PUB_JPOS_START + 2
N_PUBLIC_IO = PUB_COMMIT_DIGEST + N_DIGEST
assert IO_COLS == 64 and N_PUBLIC_IO == 24


# ------------------------------------------------------------------------------------------------ the AIRs
def io_air(ext_w=None):
    """-> the io Air of the commit form: rv32io.io_air's constraints with the commit-word rows beside READ's word rows;
    its `constraint_names` maps the name of each constraint to its index"""
    from . import p3
    b = p3.AirBuilder(IO_COLS, N_PUBLIC_IO, p3.EXT_W if ext_w is None else ext_w)
    L, N = b.local, b.next
    names = {}
    named = rv32im._namer(b, names)
    b.receive(BUS_IO, IO_TUPLE, mult=Q_HEAD, mult_is_const=False)
    b.send(BUS_MEMOP, IO_MEMOP_TUPLE, mult=Q_WORD, mult_is_const=False)
    b.send(BUS_INPUT, INPUT_TUPLE, mult=Q_WORD, mult_is_const=False)          # received by the verifier
    b.send(BUS_MEMOP, IO_MEMOP_TUPLE_CW, mult=Q_CW, mult_is_const=False)
    b.send(BUS_COMMIT, COMMIT_TUPLE, mult=Q_CW, mult_is_const=False)          # received by the verifier
    for c, m in IO_RANGE:
        b.send(BUS_RANGE16, [c], mult=m, mult_is_const=False)
    head, word, act, halt, read, commit, cw = (L(c) for c in (Q_HEAD, Q_WORD, Q_ACT, Q_HALT, Q_READ, Q_COMMIT, Q_CW))
    tr = b.is_transition()
    for tag, c in (("head", Q_HEAD), ("word", Q_WORD), ("act", Q_ACT), ("halt", Q_HALT), ("read", Q_READ), ("commit", Q_COMMIT),
                   ("k", Q_K), ("k1", Q_K1), ("z", Q_Z), ("kf", Q_KF), ("zc", Q_ZC), ("zr", Q_ZR), ("hseen", Q_HSEEN), ("cw", Q_CW),
                   ("s0", Q_S0), ("s1", Q_S1), ("c0", Q_C0), ("c1", Q_C1), ("t0b", Q_T0B), ("t1b", Q_T1B)):
        named("bool " + tag, L(c) * (L(c) - 1))
    anyw, n_anyw = word + cw, N(Q_WORD) + N(Q_CW)
    named("act", act - head - anyw)
    named("call", head - halt - read - commit)                 # one-hot: no other call has a row
    named("t0", L(Q_T0) - read - commit * 2)
    named("zero", L(Q_ZERO))
    named("op16", L(Q_OP16) - word * rv32mem.EC_CODE - cw * ECR_CODE)
    named("padding", tr * (1 - act) * N(Q_ACT))
    named("first is no word", b.is_first_row() * anyw)
    # HALT and COMMIT leave a0; READ leaves GOT
    keep = halt + commit
    named("keep lo", keep * (L(Q_RES_LO) - L(Q_AD_LO)))
    named("keep hi", keep * (L(Q_RES_HI) - L(Q_AD_HI)))
    got = L(Q_GL) + L(Q_GH) * 16384
    named("got", read * (L(Q_RES_LO) + L(Q_RES_HI) * 65536 - got))          # RES_HI < 2^14 (RH4): both sides < 2^30
    for tag, c4, c in (("rh4", Q_RH4, Q_RES_HI), ("gl4", Q_GL4, Q_GL), ("pl4", Q_PL4, Q_PL), ("nl4", Q_NL4, Q_NL), ("el4", Q_EL4, Q_EL),
                       ("jl4", Q_JL4, Q_JL)):
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
    # REM: the word rows still to follow a READ head, the bytes still to come after a COMMIT head or a commit-word row
    rem, z = L(Q_REM), L(Q_Z)
    named("rem read", read * (rem - got))
    named("rem commit", commit * (rem - L(Q_B_LO) - L(Q_B_HI) * 65536))     # a1 < 2^25 (BH7)
    named("bh7", L(Q_BH7) - L(Q_B_HI) * 128)
    named("rem keep", halt * rem)
    named("rem padding", (1 - act) * rem)
    named("z", z * rem)
    named("rinv", 1 - z - rem * L(Q_RINV))
    named("word follows", tr * (n_anyw - 1 + z))
    named("rem ends", b.is_last_row() * (1 - z))
    named("word kind", tr * N(Q_WORD) * (1 - read - word))
    named("cw kind", tr * N(Q_CW) * (1 - commit - cw))
    named("rem counts", tr * N(Q_WORD) * (N(Q_REM) - rem + 1))
    named("rem bytes", tr * N(Q_CW) * (N(Q_REM) - rem + N(Q_CNT)))
    named("rem limbs", cw * (rem - L(Q_RML) - L(Q_RMH) * 65536))
    named("rmh7", L(Q_RMH7) - L(Q_RMH) * 128)
    # a word row carries its head's TS; its address is A + 4 k, from a0 & ~3 on commit-word rows
    named("word ts", tr * n_anyw * (N(Q_TS) - L(Q_TS)))
    named("first lo", tr * N(Q_WORD) * head * (N(Q_AD_LO) - L(Q_AD_LO)))
    named("first lo cw", tr * N(Q_CW) * head * (N(Q_AD_LO) + N(Q_S) - L(Q_AD_LO)))
    named("first hi", tr * n_anyw * head * (N(Q_AD_HI) - L(Q_AD_HI)))
    named("next lo", tr * n_anyw * anyw * (N(Q_AD_LO) + N(Q_K) * 65536 - L(Q_AD_LO) - 4))
    named("next hi", tr * n_anyw * anyw * (N(Q_AD_HI) + N(Q_K1) * 65536 - L(Q_AD_HI) - N(Q_K)))
    named("aligned", (read + anyw) * (L(Q_AD_LO) - L(Q_AQ) * 4))
    # which bytes of V: S .. S + CNT - 1
    slack = L(Q_T0B) + L(Q_T1B) * 2
    named("s", L(Q_S) - L(Q_S0) - L(Q_S1) * 2)
    named("cnt", L(Q_CNT) - cw - L(Q_C0) - L(Q_C1) * 2)
    named("cnt off 0", (1 - cw) * L(Q_C0))
    named("cnt off 1", (1 - cw) * L(Q_C1))
    named("fit", cw * (L(Q_S) + L(Q_CNT) + slack - 4))
    named("full", cw * (1 - z) * slack)
    named("s later", tr * N(Q_CW) * cw * N(Q_S))
    # heads in cycle order
    named("order", tr * N(Q_HEAD) * (N(Q_TS) - L(Q_TS) - 1 - N(Q_GAP_L) - N(Q_GAP_H) * 16384))
    # the stream position and the journal position
    named("pos", tr * (N(Q_POS) - L(Q_POS) - word))
    named("pos limbs", act * (L(Q_POS) - L(Q_PL) - L(Q_PH) * 16384))
    named("pos start", b.is_first_row() * (L(Q_POS) - b.public(PUB_POS_START)))
    named("pos end", b.is_last_row() * (L(Q_POS) + word - b.public(PUB_POS_END)))
    named("jpos", tr * (N(Q_JPOS) - L(Q_JPOS) - L(Q_CNT)))
    named("jpos limbs", cw * (L(Q_JPOS) - L(Q_JL) - L(Q_JH) * 16384))
    named("jpos start", b.is_first_row() * (L(Q_JPOS) - b.public(PUB_JPOS_START)))
    named("jpos end", b.is_last_row() * (L(Q_JPOS) + L(Q_CNT) - b.public(PUB_JPOS_END)))
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
    """-> (cpu, program, register, byte, range, shift, muldiv, memop, memory, io): the AIRs of one commit shard.  link:
    the memory AIR is rv32link's"""
    return (cpu_air(ext_w), program_air(ext_w), rv32.register_air(ext_w), rv32elf.byte_air(ext_w), rv32elf.range_air(ext_w),
            rv32elf.shift_air(ext_w), rv32im.muldiv_air(ext_w), rv32mem.memop_air(ext_w, io=True, commit=True),
            rv32link.memory_air(ext_w) if link else rv32mem.memory_air(ext_w), io_air(ext_w))


# ------------------------------------------------------------------------------------------------ the log
def log_of_table(io):
    """the commit log of a canonical io table: (k, 3) uint32 -- jpos, word, S | CNT << 16 of its commit-word rows"""
    t = np.asarray(io, dtype=np.int64)
    t = t[t[:, Q_CW] == 1]
    return np.stack([t[:, Q_JL] | t[:, Q_JH] << 14, t[:, Q_V_LO] | t[:, Q_V_HI] << 16, t[:, Q_S] | t[:, Q_CNT] << 16], axis=1).astype(np.uint32)


def log_root(log, log_rows, params=None):
    """the digest of a commit log at io-table height 2^log_rows -> 8 Montgomery words (rk_rv32mem_journal_root)"""
    return rv32link.journal_root(np.asarray(log, dtype=np.uint32).reshape(-1, 3), log_rows, params)


def claims_of(log):
    """what a verifier adds for a shard's commit log: p3.verify(..., claims=claims_of(log))"""
    from . import p3
    return [(BUS_COMMIT, -1, p3.to_mont(rv32link.journal_tuples(np.asarray(log, dtype=np.uint32).reshape(-1, 3))))]


def log_bytes(pub, log):
    """the shard's slice of the journal as the log gives it, or None for a log that is not well formed against the public
    values: JPOS_START <= JPOS_END < 2^30, every row 1 <= CNT and S + CNT <= 4, the positions consecutive from JPOS_START
    and ending at JPOS_END"""
    j = np.asarray(log, dtype=np.int64).reshape(-1, 3)
    if not 0 <= pub["jpos_start"] <= pub["jpos_end"] < MAX_JOURNAL:
        return None
    pos, word, sc = j.T
    s, cnt = sc & 0xFFFF, sc >> 16
    if ((cnt < 1) | (s + cnt > 4)).any():
        return None
    want = pub["jpos_start"] + np.concatenate([[0], np.cumsum(cnt)])
    if not np.array_equal(pos, want[:-1]) or int(want[-1]) != pub["jpos_end"]:
        return None
    out = bytearray()
    for w, a, c in zip(word.tolist(), s.tolist(), cnt.tolist()):
        out += int(w).to_bytes(4, "little")[a:a + c]
    return bytes(out)


def publics_of(public_mont):
    """the io table's public values (24 Montgomery words) -> rv32io.publics_of's dict (its `digest` the input slice's)
    with jpos_start, jpos_end and commit_digest (8 Montgomery words)"""
    from . import p3
    pv = np.asarray(public_mont, dtype=np.uint32).reshape(-1)
    if pv.size != N_PUBLIC_IO:
        raise ValueError("the io table of the commit form carries %d public values" % N_PUBLIC_IO)
    out = rv32io.publics_of(pv[:rv32io.N_PUBLIC_IO])
    c = p3.from_mont(pv[PUB_JPOS_START:PUB_COMMIT_DIGEST]).astype(np.int64)
    out.update(jpos_start=int(c[0]), jpos_end=int(c[1]), commit_digest=pv[PUB_COMMIT_DIGEST:].copy())
    return out


def check_commit_chain(publics):
    """the chaining of a commit run over its shards' io public values (publics: publics_of per shard): shard 0 writes
    the journal from byte 0, every shard from where the one before stopped.  Raises ValueError naming the shard -> the
    journal's length"""
    pos = 0
    for k, pub in enumerate(publics):
        if pub["jpos_start"] != pos:
            raise ValueError("shard %d: writes the journal from byte %d, the shards before stopped at %d" % (k, pub["jpos_start"], pos))
        if not pos <= pub["jpos_end"] < MAX_JOURNAL:
            raise ValueError("shard %d: stops writing the journal at byte %d" % (k, pub["jpos_end"]))
        pos = pub["jpos_end"]
    return pos


# ------------------------------------------------------------------------------------------------ numpy witness
def _reads(reads):
    return np.asarray(reads, dtype=np.int64).reshape(-1, 3)


def n_commit_words(a0, a1):
    """the words a COMMIT of a1 bytes from a0 reads"""
    return ((a0 & 3) + a1 + 3) >> 2 if a1 else 0


def merged_accesses(mem, reads):
    """the access list memop and the memory table see: the cycle-order merge of the access list (k, 4) and the commit
    reads (k, 3) as loads (cycle, word address, word, word) -> ((n, 4) int64, which entries are commit reads).  A COMMIT
    cycle holds only reads"""
    mem, reads = rv32mem._mem(mem), _reads(reads)
    both = np.concatenate([mem, reads[:, [0, 1, 2, 2]]])
    is_read = np.concatenate([np.zeros(mem.shape[0], dtype=bool), np.ones(reads.shape[0], dtype=bool)])
    order = np.argsort(both[:, 0], kind="stable")
    return both[order], is_read[order]


def memop_rows(cpu, merged, is_read, n_rows=None):
    """rv32mem.memop_rows(io=True) over the merged list, 65 columns: a commit read is an ECR row -- LW's witness of the
    word at its address with A the address, MI = B = 0 and R the word"""
    t, hist, byte_mult, shift_mult = rv32mem.memop_rows(cpu, merged, n_rows, io=True)
    out = np.zeros((t.shape[0], MEMOP_COLS_COMMIT), dtype=np.int64)
    out[:, :rv32mem.MEMOP_COLS] = t
    r = np.nonzero(is_read)[0]
    M = rv32mem
    # what memop_rows wrote as the store of the word: the BB bytes and their ANDs go, R comes
    for u, v in M.BYTE_PAIRS[4:]:
        np.subtract.at(byte_mult, out[r, u] << 8 | out[r, v], 1)
        byte_mult[0] += r.size
    word = out[r, M.G_W_LO] | out[r, M.G_W_HI] << 16
    out[r, M.G_SEL + 8], out[r, G_ECR], out[r, M.G_OP] = 0, 1, ECR_CODE
    out[r, M.G_B_LO], out[r, M.G_B_HI], out[r, M.G_R_LO], out[r, M.G_R_HI] = 0, 0, word & 0xFFFF, word >> 16
    out[r, M.G_BB:M.G_BB + 4] = 0
    out[r, M.G_AND + 4:M.G_AND + 6] = 0
    return out, hist, byte_mult, shift_mult


def io_rows(args, ecalls, mem, reads, n_input, pos_start=None, jpos_start=0, n_rows=None):
    """the io table of the commit form -> (table (n_rows, IO_COLS) int64, the RANGE16 counts it adds, its leading public
    values: rv32io's six, then JPOS_START and JPOS_END).  args, ecalls, mem, n_input, pos_start: as rv32io.io_rows; reads:
    the commit reads (k, 3): cycle, word address, word -- per COMMIT in ascending address order from a0 & ~3.  ValueError
    for reads that are not the COMMITs' words or a COMMIT of 2^25 bytes and more"""
    args, reads = rv32io._args(args), _reads(reads)
    base, _hist, pubs = rv32io.io_rows(args, ecalls, mem, n_input, pos_start)
    base = base[base[:, Q_ACT] == 1]
    M = 0xFFFFFFFF
    rows, at, jpos, hseen = [], 0, int(jpos_start), 0
    heads = np.nonzero(base[:, Q_HEAD] == 1)[0].tolist() + [base.shape[0]]
    for e, (cycle, t0, a0, a1, _p0) in enumerate(args.tolist()):
        blk = np.zeros((heads[e + 1] - heads[e], IO_COLS), dtype=np.int64)
        blk[:, :rv32io.IO_COLS] = base[heads[e]:heads[e + 1]]
        blk[:, Q_JPOS] = jpos
        rows.append(blk)
        hseen = int(blk[-1, Q_HSEEN])
        if t0 != COMMIT:
            continue
        if a1 >= MAX_COMMIT:
            raise ValueError("a COMMIT of 2^25 bytes or more")
        blk[0, Q_REM] = a1
        ncw = n_commit_words(a0, a1)
        mine = reads[at:at + ncw]
        want = ((a0 & ~3 & M) + 4 * np.arange(ncw, dtype=np.int64) & M) >> 2
        if mine.shape[0] != ncw or (mine[:, 0] != cycle).any() or not np.array_equal(mine[:, 1], want):
            raise ValueError("the commit reads are not the words of the COMMITs in cycle order")
        at += ncw
        w = np.zeros((ncw, IO_COLS), dtype=np.int64)
        left, ad = a1, a0 & ~3 & M
        for k in range(ncw):
            s = (a0 & 3) if k == 0 else 0
            cnt = min(4 - s, left)
            left -= cnt
            t = 4 - s - cnt
            nad = (ad + 4) & M if k else ad
            r = w[k]
            r[Q_CW] = r[Q_ACT] = 1
            r[Q_TS], r[Q_OP16] = 3 * cycle + 1, ECR_CODE
            r[Q_AD_LO], r[Q_AD_HI], r[Q_AQ] = nad & 0xFFFF, nad >> 16, (nad & 0xFFFF) >> 2
            if k:
                r[Q_K] = ((ad & 0xFFFF) + 4) >> 16
                r[Q_K1] = ((ad >> 16) + r[Q_K]) >> 16
            ad = nad
            r[Q_REM], r[Q_RML], r[Q_RMH], r[Q_RMH7] = left, left & 0xFFFF, left >> 16, 128 * (left >> 16)
            r[Q_S], r[Q_S0], r[Q_S1] = s, s & 1, s >> 1
            r[Q_CNT], r[Q_C0], r[Q_C1] = cnt, (cnt - 1) & 1, (cnt - 1) >> 1
            r[Q_T0B], r[Q_T1B] = t & 1, t >> 1
            r[Q_POS], r[Q_PL], r[Q_PH] = blk[0, Q_POS], blk[0, Q_PL], blk[0, Q_PH]
            r[Q_PL4] = 4 * r[Q_PL]
            r[Q_V_LO], r[Q_V_HI] = mine[k, 2] & 0xFFFF, mine[k, 2] >> 16
            r[Q_JPOS], r[Q_JL], r[Q_JH] = jpos, jpos & 0x3FFF, jpos >> 14
            r[Q_JL4] = 4 * r[Q_JL]
            r[Q_HSEEN] = hseen
            jpos += cnt
        if jpos >= MAX_JOURNAL:
            raise ValueError("a journal of 2^30 bytes or more")
        rows.append(w)
    if at != reads.shape[0]:
        raise ValueError("the commit reads are not the words of the COMMITs in cycle order")
    count = sum(r.shape[0] for r in rows)
    n_rows = 1 << rv32io.log_rows(count) if n_rows is None else n_rows
    t = np.zeros((n_rows, IO_COLS), dtype=np.int64)
    if rows:
        t[:count] = np.concatenate(rows)
    t[count:, Q_POS], t[count:, Q_JPOS], t[count:, Q_HSEEN] = pubs[PUB_POS_END], jpos, hseen
    t[:, Q_BH7] = 128 * t[:, Q_B_HI]
    t[:, Q_Z] = t[:, Q_REM] == 0
    t[:, Q_RINV] = rv32im._inv(t[:, Q_REM])
    hist = np.zeros(1 << 16, dtype=np.int64)
    for c, m in IO_RANGE:
        hist += np.bincount(t[t[:, m] == 1, c], minlength=1 << 16)[: 1 << 16]
    return t, hist, np.concatenate([pubs, [int(jpos_start), jpos]])


def io_publics(pubs, table_rows, stream_words, log, params=None):
    """the io table's 24 public values as the prover commits them (Montgomery words): rv32io's 14, JPOS_START, JPOS_END
    and the digest of the shard's commit log at the table's height"""
    from . import p3
    lg = table_rows.bit_length() - 1
    return np.concatenate([rv32io.io_publics(pubs[:rv32io.PUB_DIGEST], table_rows, stream_words, params), p3.to_mont(pubs[rv32io.PUB_DIGEST:]),
                           log_root(log, lg, params)])


def shard_tables(seg, data, init, final_expected, ecalls, image, mem, args, reads, n_input, pos_start=None, jpos_start=0, strict=True,
                 params=None, link=False):
    """rv32io.shard_tables of a commit shard -> (the ten canonical traces, cpu public values, register public values, the
    memory table's public values -- the journal's digest with link, else () --, the io table's public values: 24
    Montgomery words).  reads, jpos_start: rk_exec_commit_reads.  The preprocessed matrices beside them are
    prep_tables(image)"""
    tr, n, _pc_lo, _pc_hi = rv32.trace_of(seg, data)
    cpu, final, final_ts, hist, byte_mult, shift_mult, sends = rv32io.cpu_rows(tr, n, seg.end_pc, init, ecalls, mem, args, strict)
    pubs = rv32.shard_publics(seg, init, final, final_expected)
    md, h2, b2, s2 = rv32im.muldiv_rows(sends, strict=strict)
    merged, is_read = merged_accesses(mem, reads)
    if merged.shape[0] > 2 * n:
        raise ValueError("segment %d: more accesses than twice the cpu table's rows" % seg.index)
    mo, h3, b3, s3 = memop_rows(cpu, merged, is_read)
    bd, h4 = rv32mem.memory_rows(merged)
    io, h5, io_pubs = io_rows(args, ecalls, mem, reads, n_input, pos_start, jpos_start)
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
             sh[:, None], md, mo, bd, io],) + pubs + (digest, io_publics(io_pubs, io.shape[0], stream, log_of_table(io), params))
