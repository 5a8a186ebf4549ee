"""TEST INFRASTRUCTURE: the guest and the parameter sets of the linked rv32im-mem runs over many shards
(tests/test_rv32_link_runs.py, tests/test_gpu_rv32_link_runs.py).  `relay` runs five 2^13-cycle shards and plants word
histories that only a chain remembering EVERY earlier shard gets right: a word written in shard 0 and next read in
shard 3, an ecall-written word loaded in the next shard, words written in shard 1 and next read in shard 4, an ELF-image
word first touched in shard 3, and a shard in the middle (2) that touches no memory at all."""
import fri_param_sets as PS
import rv32_asm as A
from rv32_mem_programs import DATA, DATA_BLOB, HALT, WORDS, _elf  # noqa: F401  (DATA_BLOB: the image `relay` is built on)

SEED_WORD = 0x5EEDBEEF
N_FILL = 60                                          # words DATA+0x100 .. written in shard 1: its memory table has 64 rows


def _spin(n, label):
    return A.li("tp", n) + [label + ":", ("addi", "tp", "tp", -1), ("xor", "t2", "t2", "tp"), ("bne", "tp", "zero", label)]


def relay_program():
    """five shards at segment_limit_po2 = 13; see HISTORIES for what crosses which boundary"""
    p = A.li("s0", DATA) + A.li("t1", SEED_WORD)
    p += [("sw", "t1", 8, "s0"), ("sb", "t1", 1, "s0")]
    p += A.li("t0", 1) + A.li("a0", DATA + 0x40) + [("addi", "a1", "zero", 2), ("ecall",)]     # READ of 2 input words
    p += _spin(2800, "spin0")
    p += [("lw", "a2", 0x40, "s0"), ("sw", "a2", 0x48, "s0")] + [("sw", "t1", 0x100 + 4 * k, "s0") for k in range(N_FILL)]
    p += _spin(5600, "spin1")                                                                   # steps over a whole shard
    p += [("lw", "a3", 4, "s0"), ("lw", "a4", 8, "s0"), ("sh", "a4", 6, "s0")]
    p += _spin(2800, "spin2")
    p += [("lw", "a5", 0x48, "s0"), ("lw", "a6", 4, "s0"), ("lw", "a7", 0x104, "s0"), ("sw", "a7", 12, "s0")]
    return _elf(p + A.li("a0", 7) + HALT)


# what X.execute(relay_program(), INPUT, segment_limit_po2=13) gives, per shard
PO2 = 13
N_SHARDS = 5
CYCLES = (8192, 8192, 8192, 8192, 920)
ACCESSES = (4, 62, 0, 3, 4)
JOURNAL_ROWS = (4, 62, 0, 2, 4)
MEMORY_HEIGHTS = (4, 64, 2, 2, 4)
TOUCHED_WORDS = 67
FINAL_AT_12 = SEED_WORD
IMAGE_AT_4 = WORDS[1]                                # 0x80007FFF
EMPTY_SHARD = 2

# byte address -> the shards whose journal holds the word, for the words whose history crosses a gap
HISTORIES = {
    DATA + 8: (0, 3),                                # written in shard 0, read in shard 3: a gap over shards 1 and 2
    DATA + 0x40: (0, 1),                             # ecall-written in shard 0, loaded in shard 1
    DATA + 0x48: (1, 4),                             # written in shard 1, read in shard 4: a gap over shards 2 and 3
    DATA + 0x104: (1, 4),
    DATA + 4: (3, 4),                                # an image word first touched in shard 3 (lw, then sh into its upper half)
}

FAST = dict(queries=8, pow_bits=6)
# name -> (preset, overrides): SP1's, risc0's (a width-24 sponge, x^4 + 11), SP1's field under another width-16 permutation
LINK_SETS = {
    "sp1": (1, dict(FAST)),
    "risc0": (0, dict(FAST)),
    "m4_0_tables": (1, dict(FAST, **PS.PARAM_SETS["m4_0_tables"][1])),
}
