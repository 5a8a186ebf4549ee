"""TEST INFRASTRUCTURE: guest programs and ELF files for the rv32im-elf chip set's tests (tests/test_rv32_elf_chips.py,
tests/test_gpu_rv32_elf_chips.py): images of every shape the program table has to hold, a guest that rewrites its own
code, and hostile program headers."""
import struct

import rv32_asm as A

HALT = A.li("t0", 0) + [("ecall",)]
BASE, SECOND = 0x00200800, 0x00300000


def code_only_program():
    """one executable segment, no data"""
    prog = A.li("s0", 0x1234ABCD) + [("addi", "a2", "zero", 5), ("mul", "a3", "a2", "s0"), ("xor", "a4", "a3", "a2"),
                                    ("slli", "a5", "a4", 3)] + HALT
    return A.elf(A.assemble(prog)[0])


def pow2_program(words=64):
    """code only, exactly `words` (a power of two) instructions: the program table has no padding row"""
    prog = [("addi", "a2", "a2", k + 1) for k in range(words - 2)] + HALT
    code = A.assemble(prog)[0]
    assert len(code) == 4 * words and words & (words - 1) == 0
    return A.elf(code)


def one_instruction_program():
    """a single ecall with t0 = 0 (halt): a one-word image, two rows"""
    return A.elf(A.assemble([("ecall",)])[0])


def second_segment_program():
    """the first segment calls code placed in the second executable segment (at data_addr), which runs ALU and M work
    and returns: the rows of a later segment start after the first one's"""
    main = A.li("t1", SECOND) + A.li("s0", 0x8765F0A1) + [("jalr", "ra", 0, "t1"), ("add", "a6", "a4", "a5")] + A.li("a0", 7) + HALT
    far = [("addi", "a2", "zero", 9), ("mul", "a3", "a2", "s0"), ("divu", "a4", "s0", "a2"), ("and", "a5", "a3", "a4"),
           ("srli", "a5", "a5", 2), ("jalr", "zero", 0, "ra")]
    return A.elf(A.assemble(main)[0], data=A.assemble(far, base=SECOND)[0], data_addr=SECOND)


def selfmod_program():
    """stores the word of `addi a2, zero, 2` over a later `addi a2, zero, 1`, then runs it: every pc still sees one word
    within the shard, but not the ELF's"""
    new = A.encode("addi", ("a2", "zero", 2), 0, {})
    head = A.li("t1", BASE + 4 * 5) + A.li("t2", new) + [("sw", "t2", 0, "t1")]
    assert len(head) == 5
    prog = head + [("addi", "a2", "zero", 1), ("add", "a3", "a2", "a2")] + HALT
    return A.elf(A.assemble(prog)[0])


def imm_program(k):
    """programs that differ in one immediate of an instruction that executes"""
    prog = [("addi", "a2", "zero", k), ("add", "a3", "a2", "a2"), ("mul", "a4", "a3", "a2")] + A.li("a0", 7) + HALT
    return A.elf(A.assemble(prog)[0], data=b"\0" * 16)


def unused_rows_program():
    """a branch that always jumps over three instructions: image rows that never execute"""
    prog = [("addi", "a2", "zero", 3), ("beq", "zero", "zero", "over"), ("addi", "a3", "zero", 1), ("mul", "a3", "a3", "a3"),
            ("addi", "a3", "a3", 2), "over:", ("add", "a4", "a2", "a2")] + HALT
    return A.elf(A.assemble(prog)[0])


def raw_elf(segs, phnum=None, size=None):
    """an ELF32 RISC-V file with the given program headers: segs = [(vaddr, blob, flags, extra)] where extra overrides
    header fields (off, filesz, memsz)"""
    ehsize, phentsize = 52, 32
    off = ehsize + phentsize * len(segs)
    hdr = b"\x7fELF" + bytes([1, 1, 1, 0]) + bytes(8)
    hdr += struct.pack("<HHIIIIIHHHHHH", 2, 243, 1, segs[0][0] if segs else BASE, ehsize, 0, 0, ehsize, phentsize,
                       len(segs) if phnum is None else phnum, 40, 0, 0)
    ph, body = b"", b""
    for vaddr, blob, flags, extra in segs:
        f = dict(off=off + len(body), filesz=len(blob), memsz=len(blob))
        f.update(extra)
        ph += struct.pack("<IIIIIIII", 1, f["off"], vaddr, vaddr, f["filesz"], f["memsz"], flags, 4)
        body += blob
    out = hdr + ph + body
    return out if size is None else out[:size]


WORD = struct.pack("<I", 0x00000073)
HOSTILE = {
    "misaligned": raw_elf([(BASE + 2, WORD * 2, 5, {})]),
    "overlap": raw_elf([(BASE, WORD * 4, 5, {}), (BASE + 8, WORD * 4, 5, {})]),
    "overlap_padded": raw_elf([(BASE, WORD + b"\x13", 5, {}), (BASE + 4, WORD, 5, {})]),   # 5 bytes pad to 2 words
    "filesz_gt_memsz": raw_elf([(BASE, WORD * 2, 5, dict(memsz=4))]),
    "offset_past_end": raw_elf([(BASE, WORD * 2, 5, dict(off=1 << 20))]),
}
TOO_MANY = raw_elf([(BASE + 64 * k, WORD, 5, {}) for k in range(17)])
SIXTEEN = raw_elf([(BASE + 64 * k, WORD, 5, {}) for k in range(16)])
