"""TEST INFRASTRUCTURE: guests at the scale of a production shard for the rv32 witness kernels (tests/test_rv32_scale.py,
tests/test_gpu_rv32_scale.py), and a census of what a cpu table reaches of the register scans.

scatter_program: tens of thousands of accesses at pseudo-random words, so that the sorted order of the access list has
nothing to do with its list order, the runs of one word are short and there are thousands of them, over hundreds of
128-position blocks; an optional ecall READ in front adds any number of accesses at one cycle.  gap_program: registers
read again after a chosen number of rows that touch none of them, so that a read's predecessor lies in the same row,
wave, block, in the block before, or several of scan_kernel's chunks back.  loadstore_loop and big_read_program of
rv32_mem_programs.py are the other two shapes: a memop table as tall as the cpu table on sixteen words, and more
accesses than cycles."""
import numpy as np

import rv32_asm as A
from raiko_amd import rv32
from rv32_mem_programs import DATA, HALT, _elf

GAPS = [0, 1, 20, 31, 40, 63, 64, 70, 100, 127, 128, 200, 260, 400, 700, 1500]
GAP_REGS = ("a2", "a3", "a4", "a5", "a6", "a7", "s4", "s5", "s6", "s7", "s8", "s9", "s10", "s11")
CLASSES = ("init", "same row", "same wave", "same block", "previous block", "earlier block, same chunk", "previous chunk",
           "earlier chunk")


def scatter_program(loops, mask=0x3FFFC, pre_read=0):
    """`loops` times 15 rows with 5 accesses (sw, lw, sb, sh, lbu) at words an LCG picks among 2^16 from DATA on, and at
    their copies 2^29 bytes higher (bit 27 of the sort key); pre_read: an RK_ECALL_READ of that many input words to
    DATA + 0x100000 first"""
    p = []
    if pre_read:
        p += A.li("t0", 1) + A.li("a0", DATA + 0x100000) + A.li("a1", pre_read) + [("ecall",)]
    p += A.li("s0", DATA) + A.li("s1", 0x1234567) + A.li("s2", 0x9E3779B1) + A.li("s3", mask) + A.li("s4", 1 << 29) + A.li("tp", loops)
    p += ["loop:",
          ("mul", "s1", "s1", "s2"), ("addi", "s1", "s1", 1), ("and", "t1", "s1", "s3"), ("add", "t1", "t1", "s0"), ("sw", "s1", 0, "t1"),
          ("srli", "t2", "s1", 13), ("and", "t2", "t2", "s3"), ("add", "t2", "t2", "s0"), ("lw", "t3", 0, "t2"), ("sb", "s1", 1, "t2"),
          ("add", "t4", "t1", "s4"), ("sh", "t3", 2, "t4"), ("lbu", "t5", 3, "t1"), ("addi", "tp", "tp", -1), ("bne", "tp", "zero", "loop")]
    return _elf(p + A.li("a0", 7) + HALT)


def gap_program(gaps, tail_spin):
    """per gap g one of fourteen registers is written, left alone for 2 g rows of a spin that touches tp only, then read
    twice in one row, read and written; after the last a spin of 2 tail_spin rows, then reads of two of them and of gp,
    which nothing wrote"""
    p = []
    for k, g in enumerate(gaps):
        r = GAP_REGS[k % len(GAP_REGS)]
        if g:
            p += A.li("tp", g)
        p.append(("addi", r, "zero", k + 1))
        if g:
            p += ["gap%d:" % k, ("addi", "tp", "tp", -1), ("bne", "tp", "zero", "gap%d" % k)]
        p += [("add", "t1", r, r), ("sub", "t2", r, "t1"), ("add", r, r, "t2")]
    p += A.li("tp", tail_spin) + ["tail:", ("addi", "tp", "tp", -1), ("bne", "tp", "zero", "tail")]
    p += [("add", "t3", "a2", "a3"), ("add", "t4", "gp", "gp")]
    return _elf(p + A.li("a0", 7) + HALT)


def census(cpu_canonical, n):
    """where the predecessor of every register access of a canonical cpu table of n rows lies, as rows_kernel finds it:
    in the row itself, among the wave's 64 rows (the shuffle scan), the block's 128 (s_wave), the block before or an
    earlier one of the same chunk (scan_kernel's running maximum within a lane's blocks nb c / 32 .. nb (c + 1) / 32),
    the chunk before or an earlier one (cm[k][r]), or nowhere in the shard (timestamp 0) -> {class: count} over PA_TS,
    PB_TS of the active rows and PW_TS of those that write"""
    cpu = np.asarray(cpu_canonical, dtype=np.int64)
    assert cpu.shape[0] == n and n % 128 == 0
    nb = n // 128
    chunk_of = np.zeros(nb, dtype=np.int64)
    for c in range(32):
        chunk_of[nb * c // 32:nb * (c + 1) // 32] = c
    out = dict.fromkeys(CLASSES, 0)
    row = np.arange(n)
    for col, on in ((rv32.PA_TS, rv32.ACTIVE), (rv32.PB_TS, rv32.ACTIVE), (rv32.PW_TS, rv32.WR)):
        sel = (cpu[:, rv32.ACTIVE] == 1) & (cpu[:, on] == 1)
        r, pts = row[sel], cpu[sel, col]
        j = (pts - 1) // 3
        assert (pts >= 0).all() and (j[pts > 0] <= r[pts > 0]).all()
        rb, jb = r // 128, np.maximum(j, 0) // 128
        rc, jc = chunk_of[rb], chunk_of[jb]
        which = np.select([pts == 0, j == r, j // 64 == r // 64, jb == rb, jb == rb - 1, jc == rc, jc == rc - 1],
                          np.arange(7), default=7)
        for k, name in enumerate(CLASSES):
            out[name] += int((which == k).sum())
    return out
