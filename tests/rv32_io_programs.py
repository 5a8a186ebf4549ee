"""TEST INFRASTRUCTURE: the guest programs of the io form's tests (tests/test_rv32_io.py, tests/test_gpu_rv32_io.py;
raiko_amd/rv32io.py): READ with capacity 0, below, at and above what the stream holds, a READ of the exhausted stream, two
READs in one shard, READs in shards 0 and 2 with none in shard 1, writes of x5, x10 and x11 right after an ecall, COMMIT,
HALT with a non-zero exit code, one READ of many words, and more ecalls than one block of the scan holds.  Shards are
2^13 cycles.  RUNS: name -> (elf, input words)."""
import rv32_asm as A
from rv32_mem_programs import DATA, _elf

BUF = DATA + 0x40
INPUT6 = [0x11223344, 0x80FF7F01, 0xDEADBEEF, 0x00000044, 0xFFFFFFFF, 0x00010000]


def _call(t0, a0, a1):
    return A.li("t0", t0) + A.li("a0", a0) + A.li("a1", a1) + [("ecall",)]


def halt(code):
    return _call(0, code, 0)


def reads_program():
    """on six input words: READ of capacity 0; of 2 (less than what is left) -- right after it x5, x11 and x10 are written, so
    that each write's predecessor is the ecall row's access --; of 4 (exactly what is left); of 3 from the exhausted
    stream (GOT 0); loads of what arrived; COMMIT of 8 bytes; HALT with exit code 5"""
    p = _call(1, BUF, 0) + _call(1, BUF, 2)
    p += [("addi", "t0", "zero", 1), ("addi", "a1", "zero", 4), ("lui", "a0", (BUF + 8) >> 12), ("addi", "a0", "a0", (BUF + 8) & 0xFFF), ("ecall",)]
    p += [("add", "s2", "a0", "zero")] + _call(1, BUF + 0x20, 3) + [("add", "s3", "a0", "zero")]
    p += A.li("s0", BUF) + [("lw", "a2", 0, "s0"), ("lw", "a3", 4, "s0"), ("lw", "a4", 20, "s0"), ("lbu", "a5", 9, "s0")]
    p += _call(2, BUF, 8)
    return _elf(p + halt(5))


def short_program():
    """a READ of capacity 10 from six words (a short read: GOT 6), then HALT with a 32-bit exit code"""
    return _elf(_call(1, BUF, 10) + [("add", "s2", "a0", "zero")] + halt(0x12345678))


def three_shard_program(spin=6000):
    """a READ in shard 0, a spin loop over the whole of shard 1 (an io table of padding only: POS is carried through it),
    a READ in shard 2"""
    p = _call(1, BUF, 2) + A.li("tp", spin)
    p += ["spin:", ("addi", "tp", "tp", -1), ("xor", "t2", "t2", "tp"), ("bne", "tp", "zero", "spin")]
    p += _call(1, BUF + 8, 3) + A.li("s0", BUF) + [("lw", "a2", 0, "s0"), ("lw", "a3", 16, "s0")]
    return _elf(p + halt(9))


def big_read_program(words):
    """one READ of `words` words, then HALT: 2 + words io rows"""
    return _elf(_call(1, DATA + 0x1000, words) + halt(1))


def halt_only_program():
    """HALT and nothing else: an io table of 2 rows"""
    return _elf(halt(3))


def many_calls_program(calls):
    """`calls` COMMITs of no bytes in a loop, then HALT: calls + 1 head rows"""
    p = A.li("tp", calls) + A.li("t0", 2) + A.li("a0", BUF) + A.li("a1", 0)
    p += ["again:", ("ecall",), ("addi", "tp", "tp", -1), ("bne", "tp", "zero", "again")]
    return _elf(p + halt(0))


def no_halt_words(n):
    return [(0x9E3779B9 * (k + 1)) & 0xFFFFFFFF for k in range(n)]


RUNS = {
    "reads": (reads_program, INPUT6),
    "short": (short_program, INPUT6),
    "three": (three_shard_program, INPUT6),
    "empty": (reads_program, []),                           # every READ of an empty stream: GOT 0
    "halt": (halt_only_program, INPUT6),                    # io table of 2 rows
    "big125": (lambda: big_read_program(125), no_halt_words(125)),   # 127 rows: the tallest one-block io table (128)
    "big200": (lambda: big_read_program(200), no_halt_words(300)),   # 202 rows: a second block; the READ's words span both
    "many": (lambda: many_calls_program(130), INPUT6),      # 131 heads: a second block of io_offsets_kernel, mscan_kernel's second chunk
}
