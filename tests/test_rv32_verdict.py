"""What the rv32 shard driver returns for a device error word (shard_verdict, raiko_amd/csrc/rv32_rows.hpp) on the CPU.
Bits 8, 16, 32 and 64 are internal-consistency flags that no honest GPU run sets, so the GPU suite cannot reach the
precedence among the bits; here every chip set's answer to every single bit, to the pairs where precedence decides and to
the two count comparisons is checked against a table written out by hand from the driver's statuses and texts.  The
function runs as a program of its own (tests/emul/emul_rv32_verdict.cpp) under AddressSanitizer and UBSan."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHIP_SETS = ["rv32i", "rv32i-cf", "rv32im", "rv32im-elf", "rv32im-mem", "io", "commit"]      # rv32::ChipSet, in order
INVALID, INTERNAL = -1, -6

OK = (0, "")
TWO = (INVALID, "rk_exec_rv32_shard_device: a pc executed with two instruction words in one shard")
SIDE = (INVALID, "rk_exec_rv32_shard_device: trace and side list disagree")
IMG_WORD = (INVALID, "rk_exec_rv32elf_shard_device: an executed word is not the program image's word at its pc")
IMG_PC = (INVALID, "rk_exec_rv32elf_shard_device: a pc executed outside the program image")
M = (INTERNAL, "rk_exec_rv32im_shard_device: an M result or the muldiv row count is not the executor's")
ACCESS = (INTERNAL, "rk_exec_rv32mem_shard_device: an access is not the one its instruction names")
HEADS = (INTERNAL, "rk_exec_rv32mem_shard_device: the distinct words on the device are not the host's")
IO_LIST = (INVALID, "rk_exec_rv32io_shard_device: the ecall side list is not the trace's ecalls")
COMMIT_READ = (INVALID, "rk_exec_rv32commit_shard_device: a commit read is not the word of its call")

# error word -> the verdict per chip set, in CHIP_SETS order, the counts agreeing
BITS = {
    0:       [OK, OK, OK, OK, OK, OK, OK],
    1:       [TWO, TWO, TWO, IMG_WORD, IMG_WORD, IMG_WORD, IMG_WORD],
    2:       [SIDE, SIDE, SIDE, SIDE, SIDE, SIDE, SIDE],
    4:       [SIDE, SIDE, SIDE, IMG_PC, IMG_PC, IMG_PC, IMG_PC],
    8:       [OK, OK, M, M, M, M, M],
    16:      [OK, OK, M, M, M, M, M],
    32:      [OK, OK, M, M, ACCESS, ACCESS, ACCESS],
    64:      [OK, OK, M, M, HEADS, HEADS, HEADS],
    128:     [OK, OK, M, M, M, M, M],
    256:     [OK, OK, M, M, M, IO_LIST, IO_LIST],
    512:     [OK, OK, M, M, M, M, COMMIT_READ],
    256 | 1: [TWO, TWO, TWO, IMG_WORD, IMG_WORD, IO_LIST, IO_LIST],
    32 | 1:  [TWO, TWO, TWO, IMG_WORD, ACCESS, ACCESS, ACCESS],
    64 | 8:  [OK, OK, M, M, HEADS, HEADS, HEADS],
    1 | 4:   [TWO, TWO, TWO, IMG_WORD, IMG_WORD, IMG_WORD, IMG_WORD],
}
# a clean word, the device's count of muldiv rows / of distinct words not the host's
M_COUNT_OFF = [OK, OK, M, M, M, M, M]
HEADS_OFF = [OK, OK, OK, OK, HEADS, HEADS, HEADS]


@pytest.fixture(scope="module")
def verdict_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the verdict program")
    exe = str(tmp_path_factory.mktemp("emul_rv32_verdict") / "emul_rv32_verdict")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "emul", "emul_rv32_verdict.cpp")],
                   check=True, capture_output=True)
    return exe


def verdicts(exe, cases):
    """cases: (chip set index, bits, m_total, m_count, heads, mem_words) -> (the ShardErr values, [(status, message)])"""
    r = subprocess.run([exe], input="".join("%d %d %d %d %d %d\n" % c for c in cases), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = r.stdout.split("\n")
    assert len(lines) == len(cases) + 2 and lines[-1] == ""
    out = []
    for line in lines[1:-1]:
        status, message = line.split("\t")
        out.append((int(status), message))
    return [int(x) for x in lines[0].split()], out


def test_the_error_bits_keep_their_values(verdict_exe):
    names, _ = verdicts(verdict_exe, [])
    assert names == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]


@pytest.mark.parametrize("cs", range(7), ids=CHIP_SETS)
def test_verdict_of_every_bit_and_of_the_pairs_where_precedence_decides(verdict_exe, cs):
    # the counts agree: 5 muldiv rows, 9 distinct words on both sides
    _, got = verdicts(verdict_exe, [(cs, bits, 5, 5, 9, 9) for bits in BITS])
    for bits, g in zip(BITS, got):
        assert g == BITS[bits][cs], (CHIP_SETS[cs], bits)


@pytest.mark.parametrize("cs", range(7), ids=CHIP_SETS)
def test_verdict_of_a_clean_word_with_counts_that_differ(verdict_exe, cs):
    _, got = verdicts(verdict_exe, [(cs, 0, 4, 5, 9, 9), (cs, 0, 6, 5, 9, 9), (cs, 0, 5, 5, 8, 9), (cs, 0, 5, 5, 10, 9),
                                    (cs, 0, 0, 0, 0, 0)])
    assert got == [M_COUNT_OFF[cs], M_COUNT_OFF[cs], HEADS_OFF[cs], HEADS_OFF[cs], OK], CHIP_SETS[cs]
