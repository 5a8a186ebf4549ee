"""TEST INFRASTRUCTURE: the guest programs of the rv32im-mem chip set's tests (tests/test_rv32_mem_chips.py,
tests/test_gpu_rv32_mem_chips.py): every load and store at every legal byte offset and on the sign edges, partial stores
into words whose other bytes are set, addresses that differ only in high bits, an address sum that wraps 2^32, a load
into x0, words written by an ecall, a run of two shards, guests with a chosen number of accesses, and a plain-Python
replay of a guest's data accesses (the reference for rk_exec_mem_accesses)."""
import struct

import rv32_asm as A

HALT = A.li("t0", 0) + [("ecall",)]
DATA = 0x00300000
M = 0xFFFFFFFF
# word 0: bytes 0x7f 0x80 0x01 0xff; word 1: halves 0x7fff 0x8000; word 2: nonzero everywhere; word 3: zero
WORDS = (0xFF01807F, 0x80007FFF, 0xA1B2C3D4, 0x00000000)
DATA_BLOB = struct.pack("<4I", *WORDS)


def _elf(prog, data=DATA_BLOB):
    return A.elf(A.assemble(prog)[0], data=data, data_addr=DATA)


def ops_program():
    """each of the eight ops at every legal byte offset: loads of bytes 0x7f / 0x80 and halves 0x7fff / 0x8000, SB and SH
    into a word whose other bytes are nonzero, a store followed by a load of the same word, the load of a word that was
    never stored (outside the data image: it reads 0)"""
    p = A.li("s0", DATA) + A.li("s1", 0x8765F0A1)
    regs = ("a2", "a3", "a4", "a5", "a6", "a7")
    k = 0
    for op in ("lb", "lbu"):
        for off in range(4):
            p.append((op, regs[k % 6], off, "s0"))
            k += 1
    for op in ("lh", "lhu"):
        for off in (0, 2, 4, 6):
            p.append((op, regs[k % 6], off, "s0"))
            k += 1
    p.append(("lw", "a2", 0, "s0"))
    p.append(("lw", "a3", 4, "s0"))
    for off in range(4):                               # SB into word 2 (0xA1B2C3D4), read back after each
        p += [("sb", "s1", 8 + off, "s0"), ("lw", regs[off], 8, "s0")]
    for off in (0, 2):                                 # SH into word 2 again
        p += [("sh", "s1", 8 + off, "s0"), ("lw", regs[off], 8, "s0"), ("lhu", "a6", 8 + off, "s0")]
    p += [("sw", "s1", 12, "s0"), ("lw", "a2", 12, "s0"), ("lb", "a3", 15, "s0"), ("lh", "a4", 14, "s0")]
    p += [("lw", "a5", 0x100, "s0"), ("lbu", "a6", 0x103, "s0")]           # never stored
    p += [("sb", "zero", 0, "s0"), ("lb", "a7", 0, "s0"), ("add", "a7", "a7", "a2")]
    return _elf(p + A.li("a0", 7) + HALT)


def far_program():
    """two addresses that differ only above bit 16 (DATA, DATA + 2^16 + ...) and two that differ only above bit 24"""
    p = A.li("s0", DATA) + A.li("s1", DATA + (1 << 16)) + A.li("s2", DATA + (1 << 24)) + A.li("s3", DATA + (1 << 29))
    p += A.li("t1", 0x11111111) + A.li("t2", 0x22222222) + A.li("t3", 0x33333333) + A.li("t4", 0x44444444)
    p += [("sw", "t1", 0, "s0"), ("sw", "t2", 0, "s1"), ("sw", "t3", 0, "s2"), ("sw", "t4", 0, "s3")]
    p += [("lw", "a2", 0, "s0"), ("lw", "a3", 0, "s1"), ("lw", "a4", 0, "s2"), ("lw", "a5", 0, "s3"),
          ("sb", "t2", 1, "s2"), ("lhu", "a6", 0, "s2"), ("lw", "a7", 0, "s0")]
    return _elf(p + A.li("a0", 7) + HALT)


def wrap_program():
    """an address sum that wraps 2^32: rs1 = 0xfffffffc, imm = 8 -> address 4; and a negative immediate"""
    p = A.li("s0", 0xFFFFFFFC) + A.li("t1", 0xCAFEF00D) + [("sw", "t1", 8, "s0"), ("lw", "a2", 8, "s0"), ("lbu", "a3", 9, "s0")]
    p += A.li("s1", DATA + 8) + [("lw", "a4", -8, "s1"), ("sh", "t1", -2, "s1"), ("lw", "a5", -4, "s1")]
    return _elf(p + A.li("a0", 7) + HALT)


def x0_program():
    """loads into x0 (no access is recorded, nothing is sent) among loads that write"""
    p = A.li("s0", DATA) + [("lw", "zero", 0, "s0"), ("lw", "a2", 0, "s0"), ("lb", "zero", 1, "s0"), ("lhu", "zero", 2, "s0"),
                            ("sw", "a2", 12, "s0"), ("lw", "zero", 12, "s0"), ("lw", "a3", 12, "s0")]
    return _elf(p + A.li("a0", 7) + HALT)


def ecall_read_program():
    """RK_ECALL_READ of three words, then loads of them (and a store over one, and a second read of one word)"""
    p = A.li("t0", 1) + A.li("a0", DATA + 0x40) + [("addi", "a1", "zero", 3), ("ecall",)]
    p += A.li("s0", DATA + 0x40) + [("lw", "a2", 0, "s0"), ("lw", "a3", 4, "s0"), ("lw", "a4", 8, "s0"), ("lbu", "a5", 5, "s0"),
                                    ("sw", "a2", 4, "s0"), ("lw", "a6", 4, "s0")]
    p += A.li("a0", DATA + 0x44) + [("addi", "a1", "zero", 1), ("ecall",), ("lw", "a7", 4, "s0"), ("lw", "a6", 12, "s0")]
    return _elf(p + A.li("a0", 7) + HALT)


def two_shard_program(spin=3000):
    """stores in the first 2^13-cycle shard, spins past its end, loads what it stored in the second"""
    p = A.li("s0", DATA) + A.li("t1", 0x5EEDBEEF) + [("sw", "t1", 8, "s0"), ("sb", "t1", 1, "s0")] + A.li("tp", spin)
    p += ["spin:", ("addi", "tp", "tp", -1), ("xor", "t2", "t2", "tp"), ("bne", "tp", "zero", "spin")]
    p += [("lw", "a2", 8, "s0"), ("lw", "a3", 0, "s0"), ("sw", "a3", 12, "s0"), ("lhu", "a4", 14, "s0")]   # no later row reads a2 (x12), as a register or as the rs2 field of an immediate
    return _elf(p + A.li("a0", 7) + HALT)


def count_program(count, distinct=False):
    """exactly `count` recorded accesses: stores and loads alternating, all at one word (one boundary row, one long
    chain), or -- distinct -- every access at a word of its own (the memory table as tall as memop)"""
    assert not distinct or 4 * count < 2048            # the 12-bit immediate
    p = A.li("s0", DATA) + A.li("t1", 0x01020304)
    for k in range(count):
        off = 4 * k if distinct else 0
        p.append(("sw", "t1", off, "s0") if k % 2 == 0 else ("lw", "a2", off, "s0"))
        p.append(("addi", "t1", "t1", 1))
    return _elf(p + A.li("a0", 7) + HALT)


def store_imm_program(imm):
    """programs that differ in the immediate of one store that executes"""
    p = A.li("s0", DATA) + A.li("t1", 0x0BADCAFE) + [("sw", "t1", imm, "s0"), ("lw", "a2", imm, "s0"), ("lb", "a3", 1, "s0")]
    return _elf(p + A.li("a0", 7) + HALT)


def forge_program():
    """a store, then a load of the same word into a register nothing reads afterwards, then a halt that leaves a0: a
    forged load result changes no later row"""
    p = A.li("s0", DATA) + A.li("t1", 0x13572468) + [("sw", "t1", 8, "s0"), ("lw", "a5", 8, "s0"), ("lb", "a4", 1, "s0"),
                                                     ("lh", "a3", 6, "s0"), ("sb", "t1", 13, "s0")]
    p += A.li("t0", 1) + A.li("a0", DATA + 0x40) + [("addi", "a1", "zero", 2), ("ecall",)]
    return _elf(p + A.li("a0", 7) + HALT)


def big_read_program(words):
    """one RK_ECALL_READ of `words` input words: more recorded accesses than cycles"""
    p = A.li("t0", 1) + A.li("a0", DATA + 0x1000) + A.li("a1", words) + [("ecall",)]
    return _elf(p + A.li("a0", 7) + HALT)


def loadstore_loop(loops):
    """a loop whose every row but two is a load or a store: the memop table is as tall as the cpu table"""
    body = []
    for k in range(16):
        body += [("sw", "t1", 4 * k, "s0"), ("lw", "t1", 4 * ((k + 5) % 16), "s0"), ("sb", "t1", 4 * k + 1, "s0"),
                 ("lhu", "t2", 4 * ((k + 9) % 16) + 2, "s0")]
    p = A.li("s0", DATA + 0x100) + A.li("t1", 0x9E3779B9) + A.li("tp", loops)
    p += ["loop:"] + body + [("addi", "tp", "tp", -1), ("bne", "tp", "zero", "loop")]
    return _elf(p + A.li("a0", 7) + HALT)


GUESTS = {"ops": ops_program, "far": far_program, "wrap": wrap_program, "x0": x0_program, "ecall": ecall_read_program}


# ---- the replay: the data accesses of a guest in plain Python, from the executed trace alone
def replay(elf, tr, regs, ecalls, input_words, memory=None, in_pos=0):
    """tr: dict of arrays over a segment's executed cycles (ins, a, b, res, wr); regs: the 32 registers at its start;
    ecalls: its (cycle, a0 after) rows; memory: {word address: word} carried between shards (the ELF's PT_LOAD bytes
    when None) -> ([(cycle, word address, before, after)], memory, in_pos).  The registers are tracked through the rows'
    written values, so an ecall READ is replayed from t0 / a0 / a1 as they stand at its row"""
    if memory is None:
        memory = {}
        phoff, = struct.unpack_from("<I", elf, 28)
        phentsize, phnum = struct.unpack_from("<HH", elf, 42)
        for i in range(phnum):
            p_type, off, vaddr, _pa, filesz, _memsz, _fl = struct.unpack_from("<IIIIIII", elf, phoff + i * phentsize)
            if p_type == 1:
                for b in range(filesz):
                    w = (vaddr + b) >> 2
                    sh = 8 * ((vaddr + b) & 3)
                    memory[w] = (memory.get(w, 0) & ~(0xFF << sh)) | elf[off + b] << sh
    out = []
    sext = lambda v, bits: v - ((v >> (bits - 1)) << bits)
    x = [int(v) for v in regs]
    a0_after = {int(c): int(v) for c, v in ecalls}
    for c, (ins, a, b) in enumerate(zip(tr["ins"], tr["a"], tr["b"])):
        ins, a, b = int(ins), int(a), int(b)
        opc, f3, rd = ins & 0x7F, (ins >> 12) & 7, (ins >> 7) & 31
        assert a == x[(ins >> 15) & 31] and b == x[(ins >> 20) & 31]
        if opc == 0x03 and rd:
            w = ((a + sext(ins >> 20, 12)) & M) >> 2
            out.append((c, w, memory.get(w, 0), memory.get(w, 0)))
        elif opc == 0x23:
            addr = (a + sext((ins >> 25) << 5 | rd, 12)) & M
            w, sh = addr >> 2, 8 * (addr & 3)
            old = memory.get(w, 0)
            mask = (0xFF, 0xFFFF, M)[f3] << sh & M
            new = (old & ~mask) | (b << sh) & mask
            memory[w] = new
            out.append((c, w, old, new))
        elif ins == 0x73 and x[5] == 1:
            dst, cap = x[10], x[11]
            got = 0
            while got < cap and in_pos < len(input_words):
                w = ((dst + 4 * got) & M) >> 2
                out.append((c, w, memory.get(w, 0), int(input_words[in_pos]) & M))
                memory[w] = int(input_words[in_pos]) & M
                in_pos += 1
                got += 1
        if ins == 0x73:
            x[10] = a0_after[c]
        elif int(tr["wr"][c]):
            x[rd] = int(tr["res"][c])
    return out, memory, in_pos
