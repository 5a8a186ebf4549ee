"""TEST INFRASTRUCTURE: the guest programs of the limb tests of the io and commit forms (tests/test_rv32_io_limbs.py,
tests/test_gpu_rv32_io_limbs.py; raiko_amd/rv32io.py, raiko_amd/rv32commit.py): the guests of rv32_io_programs.py and
rv32_commit_programs.py leave every high limb and every carry of the io table at 0.  These reach them: a journal position
past 2^14 inside one call and at a shard's start (JH), a COMMIT of more than 2^16 bytes (RMH, RMH7, BH7, B_HI), an input
of more than 2^14 words read at, before and across position 2^14 (PH, NH, EH, GH and the carry C at 1 and at 2), a READ
whose capacity is 2^16 and more (FHI, the borrow KF), two ecalls more than 2^14 timestamps apart in one shard (GAP_H), and
140 calls of mixed kinds whose rows, commit words and commit bytes differ per block of the scan.  RUNS: name -> (elf, input
words); PO2: the shard size of each; EXPECT: (exit code, input words read).

Out of scope: RES_HI / RH4 on a READ (GOT >= 2^16 needs an io table of 2^17 rows: a shard of 2^16 cycles) and K1 (an
address carry out of 2^32, which no guest can reach: mem_list_ok refuses word addresses from 2^30)."""
import rv32_asm as A
from rv32_commit_programs import BIG, BLOB, _commit
from rv32_io_programs import BUF, _call, halt, no_halt_words
from rv32_mem_programs import DATA, _elf

BIG_LEN = 0x2000 + 0x10010                                  # the data image: up to past BIG + 65541 + 1


def _byte(k):
    return (37 * k + 11 + 101 * (k >> 8)) & 0xFF


# BLOB, continued with a pattern whose period is not 256: a word or a position that is off by a multiple of 256 shows
IMAGE = bytes(_byte(k) for k in range(BIG_LEN))
assert IMAGE[:len(BLOB)] == BLOB
DST = DATA + 0x1000                                         # where the long READs store


def _at(addr, n):
    return IMAGE[addr - DATA:addr - DATA + n]


def _spin(n):
    return A.li("tp", n) + ["spin:", ("addi", "tp", "tp", -1), ("xor", "t2", "t2", "tp"), ("bne", "tp", "zero", "spin")]


def j14_program():
    """COMMIT of 16381 bytes from BIG + 1, COMMIT of 9 from BIG + 2, HALT 1: JPOS passes 2^14 inside the second call"""
    return _elf(_commit(BIG + 1, 16381) + _commit(BIG + 2, 9) + halt(1), data=IMAGE[:0x2000 + 0x4010])


def j14x_program():
    """COMMIT of 16383 bytes from BIG + 1, a spin into shard 1, COMMIT of 5 from DATA + 2, HALT 2: shard 1 starts at
    journal position 16383"""
    return _elf(_commit(BIG + 1, 16383) + _spin(2800) + _commit(DATA + 2, 5) + halt(2), data=IMAGE[:0x2000 + 0x4010])


def rem16_program():
    """a spin (the shard has 2^14 cpu rows), COMMIT of 65541 bytes from BIG + 1, COMMIT of 3 from DATA + 5, HALT 3"""
    return _elf(_spin(3000) + _commit(BIG + 1, 65541) + _commit(DATA + 5, 3) + halt(3), data=IMAGE)


def carry2_program():
    """READ of 12000 words, a spin into shard 1, the same READ again, HALT 4"""
    return _elf(_call(1, DST, 12000) + _spin(2800) + _call(1, DST, 12000) + halt(4), data=BLOB)


def carry1_program():
    """READ 5, READ 3, HALT 5"""
    return _elf(_call(1, BUF, 5) + _call(1, BUF + 0x20, 3) + halt(5), data=BLOB)


def got14_program():
    """a spin (the shard has 2^14 cpu rows), READ of 16390 words, HALT 6"""
    return _elf(_spin(3000) + _call(1, DST, 16390) + halt(6), data=BLOB)


def cap16_program():
    """READ of capacity 0x10002 from 5 words, READ of capacity 0x20000 from the exhausted stream, HALT 7"""
    return _elf(_call(1, BUF, 0x10002) + _call(1, BUF, 0x20000) + halt(7), data=BLOB)


def gap14_program():
    """COMMIT of 1 byte, a spin of 6000 cycles inside the shard, COMMIT of 1 byte, HALT 8"""
    return _elf(_commit(DATA + 1, 1) + _spin(2000) + _commit(DATA + 2, 1) + halt(8), data=BLOB)


MIXED_CALLS, MIXED_INPUT = 140, 40


def mixed_call(c):
    """call c of `mixed`: (t0, a0, a1)"""
    return (1, BUF, 1) if c % 3 == 0 else (2, DATA + c % 7, c % 10)


def mixed_program(calls=MIXED_CALLS):
    """`calls` ecalls in a loop, then HALT 9: call c is a READ of 1 word to BUF when 3 | c, else a COMMIT of c % 10 bytes
    from DATA + c % 7.  On 40 input words the READs from the 41st on are short (GOT 0)"""
    p = A.li("s1", 0) + A.li("s2", calls) + A.li("s3", 3) + A.li("s4", 7) + A.li("s5", 10) + A.li("s6", DATA) + A.li("s7", BUF)
    p += ["again:", ("remu", "t1", "s1", "s3"), ("bne", "t1", "zero", "commit"),
          ("addi", "t0", "zero", 1), ("add", "a0", "s7", "zero"), ("addi", "a1", "zero", 1), ("beq", "zero", "zero", "call"),
          "commit:", ("addi", "t0", "zero", 2), ("remu", "t1", "s1", "s4"), ("add", "a0", "s6", "t1"), ("remu", "a1", "s1", "s5"),
          "call:", ("ecall",), ("addi", "s1", "s1", 1), ("bne", "s1", "s2", "again")]
    return _elf(p + halt(9), data=BLOB)


def read_too_long_program():
    """a READ of 20000 words in a shard of 2^13 cycles: more accesses and more io rows than twice the cpu table's rows"""
    return _elf(_call(1, DST, 20000) + halt(1), data=BLOB)


def commit_too_long_program():
    """a COMMIT of 70000 bytes in a shard of 2^13 cycles: 17501 commit reads"""
    return _elf(_commit(BIG + 1, 70000) + halt(1), data=BLOB)


RUNS = {
    "j14": (j14_program, []),
    "j14x": (j14x_program, []),
    "rem16": (rem16_program, []),
    "carry2": (carry2_program, no_halt_words(36000)),
    "carry1": (carry1_program, no_halt_words(16388)),
    "got14": (got14_program, no_halt_words(16400)),
    "cap16": (cap16_program, no_halt_words(5)),
    "gap14": (gap14_program, []),
    "mixed": (mixed_program, no_halt_words(MIXED_INPUT)),
}
PO2 = {name: 14 if name in ("rem16", "got14") else 13 for name in RUNS}
READ_ONLY = ("carry1", "carry2", "cap16", "got14")          # no COMMIT: they run under plain io=True as well
EXPECT = {"j14": (1, 0), "j14x": (2, 0), "rem16": (3, 0), "carry2": (4, 24000), "carry1": (5, 8), "got14": (6, 16390), "cap16": (7, 5),
          "gap14": (8, 0), "mixed": (9, MIXED_INPUT)}
SHARDS = {name: 2 if name in ("j14x", "carry2") else 1 for name in RUNS}
# refused on the host before any launch: name -> (elf, input words); shards of 2^13 cycles
REFUSED = {
    "read": (read_too_long_program, no_halt_words(20000)),
    "commit": (commit_too_long_program, []),
}


def expected_journal(name):
    """what the guest commits, worked out from its program and the data image alone"""
    if name == "j14":
        return _at(BIG + 1, 16381) + _at(BIG + 2, 9)
    if name == "j14x":
        return _at(BIG + 1, 16383) + _at(DATA + 2, 5)
    if name == "rem16":
        return _at(BIG + 1, 65541) + _at(DATA + 5, 3)
    if name == "gap14":
        return _at(DATA + 1, 1) + _at(DATA + 2, 1)
    if name == "mixed":
        return b"".join(_at(a0, a1) for t0, a0, a1 in map(mixed_call, range(MIXED_CALLS)) if t0 == 2)
    if name in READ_ONLY:
        return b""
    raise KeyError(name)
