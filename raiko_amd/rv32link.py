"""The link between the shard memories of an rv32im-mem run (rv32mem.py): INIT of every touched word is bound to the
previous shard's FINAL and, in the first shard that touches it, to the ELF's memory image.  The first of the designs a
boundary table admits -- a DIGEST of the table -- in the form that changes neither the prover's transcript nor any AIR's
hashing.  Nine tables per shard, rv32mem's, with two additions to the `memory` table:

  the journal send   a real row also sends (WL, WH, I_LO, I_HI, F_LO, F_HI) on BUS_LINK, REAL times.  No table of the
                     proof receives it: the proof's cumulative sums no longer cancel (plain rk_p3_verify_key: reason 8).
                     The verifier is handed the shard's JOURNAL -- (word address, INIT, FINAL) per touched word,
                     ascending, (k, 3) uint32 -- and adds the receiving side itself under the proof's own permutation
                     challenges (rk_p3_verify_claims): the total must be zero
  the digest         8 public values no constraint reads: the rk_mmcs_commit root of the 2^log x 6 row-major Montgomery
                     matrix of the journal's limb tuples (rows of zeros past the k real ones; log = the memory table's
                     log height as the proof header carries it), computed on the GPU by the library's commitment path
                     (rk_rv32mem_journal_device) and recomputed by the verifier on the host (rk_rv32mem_journal_root)

WHY IT IS SOUND.  Public values are observed after the trace root and BEFORE the permutation challenges are sampled, so
the journal is fixed, up to a collision of the digest, before alpha and beta exist; the LogUp identity then makes the
multiset of real boundary rows equal the journal's tuples (limbs of a real row are range-checked by rv32mem's AIR; the
journal's limbs are 14 / 16-bit by construction).  check_memory_chain replays the journals from the ELF's memory image
(rk_exec_memory_image): INIT must be the image's word, then the image's word becomes FINAL.

STILL FREE: what an ecall writes and the a0 it leaves -- unless the run is also proven with io=True (rv32io.py), which
binds both to the run's input; the journal RK_ECALL_COMMIT appends to is then what remains.  COST: the verifier's work is linear in the touched words
(digest, claim sum, replay); a succinct link (a Merkle image, shared challenges) would bind the same table and remains a
follow-up.  The FRI statements (fri_*) over a linked proof are out of scope: their captures replay rk_p3_verify_key and
stop at reason 8.

The key is rv32mem's: the preprocessed matrices and (prep_width, log_height) per table are the same, so one
setup_rv32_elf(chips="rv32im-mem") key and root serve linked and unlinked shards.

`shard_tables` builds a linked shard's tables in numpy: the yardstick for rk_rv32mem_journal_device."""
import ctypes as C

import numpy as np

from . import _lib, rv32im, rv32mem
from .rv32 import BUS_RANGE16
from .rv32mem import (B_F_HI, B_F_LO, B_FINV, B_FTS, B_GH, B_GL, B_I_HI, B_I_LO, B_REAL, B_SAME, B_WH, B_WL, B_WL4, BUS_MEMORY,
                      MEMORY_COLS, MEMORY_RANGE, bus_balance, preps_of, prep_tables)  # noqa: F401  (re-exported)

BUS_LINK = 11
LINK_TUPLE = [B_WL, B_WH, B_I_LO, B_I_HI, B_F_LO, B_F_HI]
N_DIGEST = 8
MEMORY_TABLE = 8                                   # the memory table's index among a shard's nine


def memory_air(ext_w=None):
    """rv32mem.memory_air with the journal send and the digest's 8 public values (which no constraint reads)"""
    from . import p3
    b = p3.AirBuilder(MEMORY_COLS, N_DIGEST, p3.EXT_W if ext_w is None else ext_w)
    L = b.local
    names = {}
    named = rv32im._namer(b, names)
    b.send(BUS_MEMORY, [B_WL, B_WH, B_I_LO, B_I_HI], mult=B_REAL, mult_is_const=False)          # at timestamp 0
    b.receive(BUS_MEMORY, [B_WL, B_WH, B_F_LO, B_F_HI, B_FTS], mult=B_REAL, mult_is_const=False)
    for c in MEMORY_RANGE:
        b.send(BUS_RANGE16, [c], mult=B_REAL, mult_is_const=False)
    b.send(BUS_LINK, LINK_TUPLE, mult=B_REAL, mult_is_const=False)                              # received by the verifier
    real, same = L(B_REAL), L(B_SAME)
    named("bool real", real * (real - 1))
    named("padding", b.is_transition() * (1 - real) * b.next(B_REAL))
    named("wl4", L(B_WL4) - L(B_WL) * 4)
    named("touched", real * (L(B_FTS) * L(B_FINV) - 1))
    named("bool same", same * (same - 1))
    into = b.is_transition() * b.next(B_REAL)
    named("same high", into * same * (b.next(B_WH) - L(B_WH)))
    named("ascending low", into * same * (b.next(B_WL) - L(B_WL) - 1 - L(B_GL)))
    named("ascending high", into * (1 - same) * (b.next(B_WH) - L(B_WH) - 1 - L(B_GH)))
    air = b.build()
    air.constraint_names = names
    return air


def airs(ext_w=None):
    """rv32mem.airs with the linked memory AIR in the ninth place"""
    return rv32mem.airs(ext_w)[:MEMORY_TABLE] + (memory_air(ext_w),)


# ------------------------------------------------------------------------------------------------ the journal
def journal_of_table(memory):
    """the journal of a canonical memory table (rows, 13): (k, 3) uint32 -- word address, INIT, FINAL of its real rows"""
    t = np.asarray(memory, dtype=np.int64)
    t = t[t[:, B_REAL] == 1]
    return np.stack([t[:, B_WL] | t[:, B_WH] << 14, t[:, B_I_LO] | t[:, B_I_HI] << 16, t[:, B_F_LO] | t[:, B_F_HI] << 16],
                    axis=1).astype(np.uint32)


def journal_of(mem):
    """the journal of an access list (k, 4): cycle, word address, old word, new word -> (words, 3) uint32, ascending"""
    return journal_of_table(rv32mem.memory_rows(mem)[0])


def journal_tuples(journal):
    """the limb tuples (WL, WH, I_LO, I_HI, F_LO, F_HI) of a journal: (k, 6) int64, canonical"""
    j = np.asarray(journal, dtype=np.int64).reshape(-1, 3)
    a, i, f = j.T
    return np.stack([a & 0x3FFF, a >> 14, i & 0xFFFF, i >> 16, f & 0xFFFF, f >> 16], axis=1)


def link_matrix(journal, log_rows):
    """the 2^log_rows x 6 Montgomery matrix the digest commits to: the journal's tuples, then rows of zeros"""
    from . import p3
    m = np.zeros((1 << log_rows, len(LINK_TUPLE)), dtype=np.uint32)
    t = journal_tuples(journal)
    m[:t.shape[0]] = p3.to_mont(t)
    return m


def journal_root(journal, log_rows, params=None):
    """rk_rv32mem_journal_root (host only): the digest of a journal at memory-table height 2^log_rows -> 8 Montgomery
    words.  params: an RkParams blob or None for the SP1 preset.  RkError (RK_ERR_INVALID) for more rows than the table
    has, an address >= 2^30 or addresses that do not strictly ascend"""
    lib = _lib.load()
    j = np.ascontiguousarray(journal, dtype=np.uint32).reshape(-1, 3)
    root = np.zeros(N_DIGEST, dtype=np.uint32)
    _lib.check(None, lib.rk_rv32mem_journal_root(C.byref(params) if params is not None else None, j.ctypes.data_as(_lib.u32p),
                                                 j.shape[0], int(log_rows), root.ctypes.data_as(_lib.u32p)))
    return root


def claims_of(journal):
    """what a verifier adds for a shard's journal: p3.verify(..., claims=claims_of(journal))"""
    from . import p3
    return [(BUS_LINK, -1, p3.to_mont(journal_tuples(journal)))]


def memory_image(elf: bytes):
    """rk_exec_memory_image: every word that holds a file byte of a PT_LOAD segment, as the executor's loader stores
    them -> (word addresses ascending, words): uint32 arrays"""
    lib = _lib.load()
    n = C.c_size_t(0)
    st = lib.rk_exec_memory_image(bytes(elf), len(elf), None, None, 0, C.byref(n))
    if st != _lib.RK_ERR_CAPACITY:
        _lib.check(None, st)
    addr, words = np.zeros(max(n.value, 1), dtype=np.uint32), np.zeros(max(n.value, 1), dtype=np.uint32)
    _lib.check(None, lib.rk_exec_memory_image(bytes(elf), len(elf), addr.ctypes.data_as(_lib.u32p), words.ctypes.data_as(_lib.u32p),
                                              addr.size, C.byref(n)))
    return addr[: n.value], words[: n.value]


def check_memory_chain(journals, image):
    """Replays the shards' journals, in the order check_rv32_chain binds the shards, from the ELF's memory image (image:
    memory_image(elf), or {word address: word}; zero elsewhere): for every journal row INIT must equal the image's word,
    then the image's word becomes FINAL.  Raises ValueError naming the shard and the word address -> the final image of
    the touched words {word address: word}"""
    cur = dict(image) if isinstance(image, dict) else {int(a): int(w) for a, w in zip(*image)}
    touched = {}
    for k, j in enumerate(journals):
        for a, init, fin in np.asarray(j, dtype=np.int64).reshape(-1, 3).tolist():
            have = touched.get(a, cur.get(a, 0))
            if init != have:
                raise ValueError("shard %d: word 0x%08x starts from 0x%08x, the memory before it holds 0x%08x" % (k, a << 2, init, have))
            touched[a] = fin
    return touched


# ------------------------------------------------------------------------------------------------ numpy witness
def shard_tables(seg, data, init, final_expected, ecalls, image, mem, strict=True, params=None):
    """rv32mem.shard_tables of a linked shard -> (the nine canonical traces, cpu public values, register public values,
    the memory table's public values: the digest of the shard's journal, 8 Montgomery words as the prover commits them)"""
    tables, pub_cpu, pub_reg = rv32mem.shard_tables(seg, data, init, final_expected, ecalls, image, mem, strict)
    bd = tables[MEMORY_TABLE]
    return tables, pub_cpu, pub_reg, journal_root(journal_of_table(bd), bd.shape[0].bit_length() - 1, params)
