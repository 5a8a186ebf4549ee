"""The rv32im-elf chip set: rv32im's statement (rv32im.py) with the program table bound to the ELF.  Everything a shard
cannot change -- the program's (pc, word, decoded fields), the byte, range and shift tables' tuples -- is PREPROCESSED:
committed once per ELF by setup (p3.setup / rk_p3_setup) into a key whose root the verifier is given; a shard's main
trace keeps only what the shard decides.  Seven tables in rv32im's order:

  cpu, register, muldiv   rv32im's AIRs, columns and rows, unchanged (imported, not copied)
  program   width 1 (the multiplicity), prep_width 42: the 41 columns of rv32im.PROGRAM_TUPLE in that order -- exactly
            what a cpu row sends -- and VALID, one row per word of the program image, then padding rows (word 0 at pc
            0, multiplicity 0) up to a power of two >= 2; receives (PROGRAM: prep 0..40) main[0] times; the one
            constraint is mult * (1 - VALID) = 0
  byte      width 1, prep_width 4 (Y_OP, Y_X, Y_Y, Y_Z), 2^18 rows, no constraints
  range     width 1, prep_width 1 (the value), 2^16 rows, no constraints
  shift     width 1, prep_width 4 (H_K, H_X, H_LO, H_HI), 2^12 rows, no constraints

The program image: the words of every PT_LOAD segment with PF_X set, in program-header order, each segment's file
bytes zero-padded to whole words (`program_image`).  VALID is 1 where a cpu row may look the word up: its opcode is
one of rv32.OPCODES (the sum s of rv32.program_constraints) and it is not an OP word with bit 25 set that is no M word
(the op * bit25 - is_m test of rv32im.program_air).

WHAT SETUP IS TRUSTED FOR.  rv32im's program AIR proves every decoded field from the word's 32 bits inside each proof;
here no proof does: the bit, selector and partial-product columns are gone and the preprocessed rows are whatever setup
committed.  Decode correctness rests on setup: a verifier trusts a root exactly as far as it trusts whoever derived it
from the ELF (by running `prep_tables` / rk_rv32elf_prep_device on the ELF's image and committing the result).  The
reference for the matrices is `prep_tables`: the tuple columns of the full-width rows rv32im's AIRs prove consistent.
What the proof gains: every executed (pc, word) is a row of THAT image (a pc outside it, or a word a store changed,
has no row to look up), and every shard of a run looks up the same image.
Free as under rv32im: loads, stores and memory; the a0 an ecall leaves.

`shard_tables` builds a shard's seven traces in numpy: the yardstick for rk_exec_rv32elf_shard_device."""
import struct

import numpy as np

from . import rv32, rv32cf, rv32im
from .rv32 import BUS_BYTE, BUS_PROGRAM, BUS_RANGE16
from .rv32cf import BUS_SHIFT

MAX_SEGMENTS = 16
# the program table's tuple columns among rv32im's 101: rv32i's 20, rv32i-cf's twelve fields, rv32im's nine
TUPLE_COLS = list(range(20)) + list(range(rv32cf.P_EXT, rv32im.P_EXT)) + list(range(rv32im.P_EXT, rv32im.P_EXT + 9))
assert len(TUPLE_COLS) == len(rv32im.PROGRAM_TUPLE) == 41
P_VALID = len(TUPLE_COLS)                 # preprocessed column 41
PROGRAM_PREP = P_VALID + 1
BYTE_TUPLE = [rv32.Y_OP, rv32.Y_X, rv32.Y_Y, rv32.Y_Z]
SHIFT_TUPLE = [rv32cf.H_K, rv32cf.H_X, rv32cf.H_LO, rv32cf.H_HI]
RANGE_LOG_ROWS = 16


# ------------------------------------------------------------------------------------------------ the AIRs
def _lookup_air(bus, prep_width, ext_w):
    """a table that is a preprocessed tuple per row and its multiplicity as the only trace column; no constraints"""
    from . import p3
    b = p3.AirBuilder(1, 0, p3.EXT_W if ext_w is None else ext_w, prep_width=prep_width)
    b.receive(bus, [b.prep(c) for c in range(prep_width)], mult=0, mult_is_const=False)
    return b


def program_air(ext_w=None):
    from . import p3
    b = p3.AirBuilder(1, 0, p3.EXT_W if ext_w is None else ext_w, prep_width=PROGRAM_PREP)
    b.receive(BUS_PROGRAM, [b.prep(c) for c in range(P_VALID)], mult=0, mult_is_const=False)
    b.assert_zero(b.local(0) * (1 - b.prep_local(P_VALID)))
    return b.build()


def byte_air(ext_w=None):
    return _lookup_air(BUS_BYTE, 4, ext_w).build()


def range_air(ext_w=None):
    """p3.p3_range_air_prep on the RANGE16 bus"""
    return _lookup_air(BUS_RANGE16, 1, ext_w).build()


def shift_air(ext_w=None):
    return _lookup_air(BUS_SHIFT, 4, ext_w).build()


def airs(ext_w=None):
    """-> (cpu, program, register, byte, range, shift, muldiv): the AIRs of one rv32im-elf shard, in table order"""
    return (rv32im.cpu_air(ext_w), program_air(ext_w), rv32.register_air(ext_w), byte_air(ext_w), range_air(ext_w),
            shift_air(ext_w), rv32im.muldiv_air(ext_w))


# ------------------------------------------------------------------------------------------------ the program image
def program_image(elf):
    """the executable image of an ELF32 little-endian RISC-V file -> [(vaddr, words (int64 array))]: every PT_LOAD
    segment with PF_X and file bytes, in program-header order, the file bytes zero-padded to whole words.  ValueError
    for a file the executor's loader refuses, a misaligned executable segment, overlapping executable segments or more
    than MAX_SEGMENTS of them."""
    elf = bytes(elf)
    n = len(elf)
    if n < 52 or elf[:4] != b"\x7fELF":
        raise ValueError("not an ELF file")
    if elf[4] != 1 or elf[5] != 1:
        raise ValueError("not a 32-bit little-endian ELF")
    if struct.unpack_from("<H", elf, 18)[0] != 243:
        raise ValueError("not a RISC-V ELF (e_machine != 243)")
    phoff, = struct.unpack_from("<I", elf, 28)
    phentsize, phnum = struct.unpack_from("<HH", elf, 42)
    if phentsize < 32 or phoff + phentsize * phnum > n:
        raise ValueError("program headers out of range")
    image = []
    for i in range(phnum):
        p_type, off, vaddr, _paddr, filesz, memsz, flags = struct.unpack_from("<IIIIIII", elf, phoff + i * phentsize)
        if p_type != 1:
            continue
        if off + filesz > n or filesz > memsz or vaddr + memsz > 1 << 32:
            raise ValueError("PT_LOAD segment out of range")
        if not flags & 1 or filesz == 0:
            continue
        if vaddr & 3:
            raise ValueError("misaligned executable segment")
        blob = elf[off:off + filesz] + bytes(-filesz % 4)
        image.append((vaddr, np.frombuffer(blob, dtype="<u4").astype(np.int64)))
    if len(image) > MAX_SEGMENTS:
        raise ValueError("more than %d executable segments" % MAX_SEGMENTS)
    spans = sorted((v, v + 4 * w.size) for v, w in image)
    if any(a[1] > b[0] for a, b in zip(spans, spans[1:])) or (spans and spans[-1][1] > 1 << 32):
        raise ValueError("overlapping executable segments")
    return image


def image_rows(image):
    """-> (pc of every image row, its word, the program table's height: a power of two >= 2)"""
    pcs = np.concatenate([v + 4 * np.arange(w.size, dtype=np.int64) for v, w in image] + [np.zeros(0, dtype=np.int64)])
    words = np.concatenate([np.asarray(w, dtype=np.int64) for _v, w in image] + [np.zeros(0, dtype=np.int64)])
    n_rows = 2
    while n_rows < pcs.size:
        n_rows <<= 1
    return pcs, words, n_rows


def program_full_rows(image, counts=None):
    """rv32im's full-width program rows (rv32im.PROGRAM_COLS columns) over the image's (pc, word), padded with rv32im's
    padding row: what rv32im.program_air proves consistent"""
    pcs, words, n_rows = image_rows(image)
    base = rv32.program_rows(pcs, words, np.zeros(pcs.size, dtype=np.int64) if counts is None else counts, n_rows)
    ins = base[:, 2] | base[:, 3] << 16
    return np.concatenate([base, rv32cf.decode(ins), rv32im.decode(ins)], axis=1)


def valid_of(full):
    """VALID of full-width program rows: the opcode-class sum s, minus the OP words with bit 25 set that are no M word"""
    s = full[:, rv32.P_OPC:rv32.P_OPC + 11].sum(axis=1)
    bad = full[:, rv32.P_OPC + rv32.O_OP] * full[:, rv32.P_BITS + 25] - full[:, rv32im.P_EXT + 8]
    return s * (1 - bad)


def prep_tables(image):
    """the four canonical preprocessed matrices -> (program (rows, 42), byte (2^18, 4), range (2^16, 1), shift (2^12, 4)):
    the tuple columns of the existing full-width numpy rows"""
    full = program_full_rows(image)
    prog = np.concatenate([full[:, TUPLE_COLS], valid_of(full)[:, None]], axis=1)
    return (prog, rv32.byte_rows()[:, BYTE_TUPLE], np.arange(1 << RANGE_LOG_ROWS, dtype=np.int64)[:, None],
            rv32cf.shift_rows()[:, SHIFT_TUPLE])


def program_mult(pcs, inss, image):
    """how often a shard ran every image row -> (program table height,) int64.  ValueError when an executed (pc, word)
    is not the image's word at that pc: a pc outside every executable segment, or a word changed by a store"""
    ipc, iword, n_rows = image_rows(image)
    mult = np.zeros(n_rows, dtype=np.int64)
    pcs, inss = np.asarray(pcs, dtype=np.int64), np.asarray(inss, dtype=np.int64)
    if pcs.size == 0:
        return mult
    order = np.argsort(ipc, kind="stable")
    at = np.searchsorted(ipc[order], pcs)
    at = np.minimum(at, max(ipc.size - 1, 0))
    if ipc.size == 0 or not np.array_equal(ipc[order][at], pcs):
        raise ValueError("a pc executed outside the program image")
    rows = order[at]
    if not np.array_equal(iword[rows], inss):
        raise ValueError("an executed word is not the program image's word at its pc")
    return mult + np.bincount(rows, minlength=n_rows)


def shard_tables(seg, data, init, final_expected, ecalls, image):
    """the seven canonical traces of one executed segment -> ([cpu, program, register, byte, range, shift, muldiv]
    canonical int64 arrays: the four lookup tables a multiplicity column each, cpu public values, register public
    values); the preprocessed matrices beside them are prep_tables(image)"""
    tr, n, _pc_lo, _pc_hi = rv32.trace_of(seg, data)
    cpu, final, final_ts, hist, byte_mult, shift_mult, sends = rv32im.cpu_rows(tr, n, seg.end_pc, init, ecalls)
    pubs = rv32.shard_publics(seg, init, final, final_expected)
    md, h2, b2, s2 = rv32im.muldiv_rows(sends)
    prog = program_mult(tr["pc"], tr["ins"], image)
    byt = np.zeros(1 << rv32.BYTE_LOG_ROWS, dtype=np.int64)
    byt[: 3 << 16] = byte_mult + b2
    sh = np.zeros(1 << rv32cf.SHIFT_LOG_ROWS, dtype=np.int64)
    sh[: rv32cf.SHIFT_USED] = shift_mult + s2
    return ([cpu, prog[:, None], rv32.register_rows(init, final, final_ts), byt[:, None], (hist + h2)[:, None],
             sh[:, None], md],) + pubs


def preps_of(image):
    """prep_tables in table order: None for the cpu, register and muldiv tables"""
    prog, byt, rng, sh = prep_tables(image)
    return [None, prog, None, byt, rng, sh, None]
