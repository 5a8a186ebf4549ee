"""TEST INFRASTRUCTURE: the guest programs of the commit form's tests (tests/test_rv32_commit.py,
tests/test_gpu_rv32_commit.py; raiko_amd/rv32commit.py): COMMIT of 0 bytes, of 1 byte at each offset, of 2 bytes across a
word boundary, of 4 aligned bytes, of 7 bytes from offset 1, of 9 from offset 0, across a 2^16 address boundary, of a
buffer a READ filled, of a word an SB changed in between, twice of one word, in shards 0 and 2 with none in shard 1, of
513 bytes from offset 3 (129 word rows) and 130 COMMITs of one byte.  Shards are 2^13 cycles.  RUNS: name -> (elf, input
words)."""
import struct

import rv32_asm as A
from rv32_io_programs import BUF, INPUT6, _call, halt
from rv32_mem_programs import DATA, _elf

# the data image: 64 bytes with every byte distinct, so that a wrong byte offset shows
BLOB = bytes((37 * k + 11) & 0xFF for k in range(64))
EDGE = DATA + 0x10000 - 6                                  # 6 bytes below a 2^16 address boundary
BIG = DATA + 0x2000


def _commit(addr, n):
    return _call(2, addr, n)


def small_program():
    """COMMIT of 0 bytes, of 1 byte at offsets 0..3, of 2 bytes from offset 3, of 4 aligned bytes, of 7 bytes from
    offset 1, of 9 bytes from offset 0; HALT 5"""
    p = _commit(DATA + 5, 0)
    for off in range(4):
        p += _commit(DATA + 8 + off, 1)
    p += _commit(DATA + 3, 2) + _commit(DATA + 16, 4) + _commit(DATA + 21, 7) + _commit(DATA + 32, 9)
    return _elf(p + halt(5), data=BLOB)


def edge_program():
    """stores around a 2^16 address boundary, then a COMMIT of 12 bytes from 6 bytes below it: the address carry"""
    p = A.li("s0", DATA + 0x10000) + A.li("t1", 0x44332211) + A.li("t2", 0x88776655)
    p += [("sw", "t1", -8, "s0"), ("sw", "t2", -4, "s0"), ("sw", "t1", 0, "s0"), ("sw", "t2", 4, "s0")]
    return _elf(p + _commit(EDGE, 12) + halt(1), data=BLOB)


def read_commit_program():
    """a READ of 4 words into a buffer, then a COMMIT of 13 of its bytes from offset 2"""
    return _elf(_call(1, BUF, 4) + _commit(BUF + 2, 13) + halt(2), data=BLOB)


def sb_program():
    """a COMMIT of a word, an SB into it, a COMMIT of the same word (two COMMITs of one word; the second sees the store),
    and a third of its upper half"""
    p = _commit(DATA + 4, 4) + A.li("s0", DATA) + A.li("t1", 0xEE) + [("sb", "t1", 6, "s0")]
    return _elf(p + _commit(DATA + 4, 4) + _commit(DATA + 6, 2) + halt(3), data=BLOB)


def three_shard_program(spin=6000):
    """a COMMIT in shard 0, a spin loop over the whole of shard 1 (JPOS is carried through an io table of padding), a
    COMMIT in shard 2"""
    p = _commit(DATA + 1, 6) + A.li("tp", spin)
    p += ["spin:", ("addi", "tp", "tp", -1), ("xor", "t2", "t2", "tp"), ("bne", "tp", "zero", "spin")]
    return _elf(p + _commit(DATA + 9, 5) + halt(9), data=BLOB)


def big_program():
    """one COMMIT of 513 bytes from offset 3: 129 commit-word rows, which span two blocks of the io rows kernel"""
    p = A.li("s0", BIG) + A.li("t1", 0xA5C3E187) + [("sw", "t1", 0, "s0"), ("sw", "t1", 256, "s0"), ("sw", "t1", 512, "s0")]
    return _elf(p + _commit(BIG + 3, 513) + halt(1), data=BLOB)


def many_program(calls=130):
    """`calls` COMMITs of 1 byte each at ascending addresses, then HALT: calls + 1 heads and `calls` commit-word rows"""
    p = A.li("tp", calls) + A.li("t0", 2) + A.li("a0", DATA) + A.li("a1", 1)
    p += ["again:", ("ecall",), ("addi", "a0", "a0", 1), ("addi", "tp", "tp", -1), ("bne", "tp", "zero", "again")]
    return _elf(p + halt(0), data=BLOB + BLOB[::-1] + BLOB)


RUNS = {
    "small": (small_program, []),
    "edge": (edge_program, []),
    "read": (read_commit_program, INPUT6),
    "sb": (sb_program, []),
    "three": (three_shard_program, []),
    "big": (big_program, []),
    "many": (many_program, []),
}


def expected_journal(name):
    """what the guest commits, worked out from its program and the data image alone"""
    mem = bytearray(0x3000)
    mem[:len(BLOB)] = BLOB
    at = lambda addr, n: bytes(mem[addr - DATA:addr - DATA + n])
    if name == "small":
        return b"".join(at(DATA + 8 + k, 1) for k in range(4)) + at(DATA + 3, 2) + at(DATA + 16, 4) + at(DATA + 21, 7) + at(DATA + 32, 9)
    if name == "edge":
        return struct.pack("<4I", 0x44332211, 0x88776655, 0x44332211, 0x88776655)[2:14]
    if name == "read":
        return struct.pack("<4I", *INPUT6[:4])[2:15]
    if name == "sb":
        after = bytearray(at(DATA + 4, 4))
        after[2] = 0xEE
        return at(DATA + 4, 4) + bytes(after) + bytes(after[2:4])
    if name == "three":
        return at(DATA + 1, 6) + at(DATA + 9, 5)
    if name == "big":
        for off in (0, 256, 512):
            mem[0x2000 + off:0x2000 + off + 4] = struct.pack("<I", 0xA5C3E187)
        return at(BIG + 3, 513)
    if name == "many":
        return (BLOB + BLOB[::-1] + BLOB)[:130]
    raise KeyError(name)
