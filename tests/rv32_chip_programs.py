"""TEST INFRASTRUCTURE: guest programs for the rv32i chip set tests (every constrained opcode at its edge values, the free
ones beside them, ecall READ, a loop long enough for several shards) and a helper that forges a table cell."""
import numpy as np

import rv32_asm as A

HALT = A.li("t0", 0) + [("ecall",)]


def alu_program(loops=1):
    """every constrained op at edge values; `loops` passes of a loop of them, so that a run spans several shards"""
    body = []
    body += A.li("s0", 0x7FFFFFFF) + [("addi", "s1", "zero", 1), ("add", "t1", "s0", "s1")]        # 0x7fffffff + 1
    body += A.li("s2", 0x80000000) + [("sub", "t2", "s2", "s1"), ("addi", "t3", "s2", -1)]           # 0x80000000 - 1
    body += [("addi", "t4", "zero", -2048), ("addi", "t4", "t4", 2047), ("add", "zero", "s0", "s1"),  # rd = x0
             ("add", "t5", "t5", "t5"), ("sub", "t6", "t6", "t6")]                                   # rd = rs1 = rs2
    body += [("slt", "a2", "s2", "s0"), ("slt", "a3", "s0", "s2"), ("sltu", "a4", "s2", "s0"), ("sltu", "a5", "s0", "s2"),
             ("slti", "a6", "s2", -1), ("sltiu", "a7", "s1", -1), ("slti", "a6", "s0", 5), ("sltiu", "a7", "zero", 0),
             ("slt", "a2", "s1", "s1")]
    body += A.li("s3", 0xF0F0A55A) + [("xor", "s4", "s3", "s0"), ("or", "s5", "s3", "s1"), ("and", "s6", "s3", "s2"),
                                       ("xori", "s7", "s3", -1), ("ori", "s8", "s3", -256), ("andi", "s9", "s3", 0x7F0),
                                       ("xor", "s10", "s10", "s10")]
    body += [("lui", "s11", 0xFFFFF), ("auipc", "t1", 0x80000), ("auipc", "t2", 0)]
    body += [("jal", "ra", "j1"), "j1:", ("auipc", "t3", 0), ("jalr", "t4", 12, "t3"), ("addi", "zero", "zero", 0), "j2:"]
    # free ops beside them: shifts, M, loads / stores, branches
    body += A.li("t1", 0x300000) + [("sw", "s3", 8, "t1"), ("lw", "t2", 8, "t1"), ("lbu", "t3", 9, "t1"),
                                     ("slli", "t4", "s3", 3), ("sra", "t5", "s3", "s1"), ("mul", "t6", "s3", "s0"),
                                     ("divu", "t6", "s3", "s1"), ("beq", "t2", "s3", "b1"), ("addi", "t2", "zero", 0), "b1:"]
    prog = A.li("t0", 1) + A.li("a0", 0x300100) + [("addi", "a1", "zero", 4), ("ecall",), ("add", "gp", "a0", "a0")]
    prog += A.li("tp", loops) + ["loop:"] + body + [("addi", "tp", "tp", -1), ("bne", "tp", "zero", "loop")]
    prog += A.li("a0", 7) + HALT
    code, _ = A.assemble(prog)
    return A.elf(code, data=b"\0" * 0x200)


def tables_canon(tables):
    from raiko_amd import p3
    return [p3.from_mont(t.trace).astype(np.int64) for t in tables]


def replace(tables, k, canon):
    """tables with table k's trace replaced by the canonical array `canon`"""
    from raiko_amd import p3
    out = list(tables)
    out[k] = p3.Table(tables[k].air, p3.to_mont(np.asarray(canon) % p3.P), tables[k].public_values)
    return out
