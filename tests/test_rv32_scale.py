"""The guests of tests/test_gpu_rv32_scale.py are what they claim (no GPU): the shards, cycles, accesses, distinct words
and table heights each one is run for -- a memop table as tall as the cpu table, tables of twice its height, an access
list of exactly 1 024 blocks of 128 and one past it, the cap of twice the cpu table met exactly -- and, for the register
side, that every place rows_kernel can find an access's predecessor in occurs (rv32_scale_programs.census).  At two of
the shapes the numpy witness itself is held: every bus balances, and the lane bodies of rv32_rows.hpp, walked by
tests/emul/emul_rv32_mem.cpp, write the same words."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rv32_mem_programs as GP
import rv32_scale_programs as SP
from raiko_amd import _lib, p3, rv32, rv32cf, rv32elf, rv32im, rv32mem
from raiko_amd import executor as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_INPUT = [11, 22, 33, 44]
# name -> (guest, input words, shard limit)
MEM_CASES = {
    "loadstore": (lambda: GP.loadstore_loop(1100), 0, 16),
    "scatter": (lambda: SP.scatter_program(4300), 0, 16),
    "read16000": (lambda: GP.big_read_program(16000), 16384, 13),
    "read16384": (lambda: GP.big_read_program(16384), 16384, 13),
    "blocks1024": (lambda: SP.scatter_program(8700, pre_read=87572), 140000, 17),
    "blocks1025": (lambda: SP.scatter_program(8700, pre_read=87573), 140000, 17),
}
_runs = {}


def _run(name):
    """-> (elf, execution, image, the canonical tables of shard 0), computed once"""
    if name not in _runs:
        guest, n_input, po2 = MEM_CASES[name]
        elf = guest()
        ex = X.execute(elf, list(range(1, n_input + 1)), segment_limit_po2=po2, record_trace=True)
        image = rv32elf.program_image(elf)
        (_c, data), (start, end, ecalls) = ex.witness[0], ex.rv32[0]
        canon = rv32mem.shard_tables(ex.segments[0], data, start, end, ecalls, image, ex.mem[0])[0]
        _runs[name] = (elf, ex, image, canon)
    return _runs[name]


def _shape(name):
    """-> ([(cycles, po2)] per shard, and of shard 0: accesses, distinct words, memop rows, memory rows, cpu rows)"""
    _elf, ex, _image, canon = _run(name)
    mem = ex.mem[0]
    assert int(canon[7][:, rv32mem.G_MULT].sum()) == len(mem) and int(canon[8][:, rv32mem.B_REAL].sum()) == np.unique(mem[:, 1]).size
    return [(s.cycles, s.po2) for s in ex.segments], (len(mem), np.unique(mem[:, 1]).size, canon[7].shape[0], canon[8].shape[0], canon[0].shape[0])


def test_loadstore_loop_fills_memop_to_the_cpu_table():
    shards, shard0 = _shape("loadstore")
    assert [c for c, _p in shards] == [65536, 7072] and shards[0][1] == 16
    assert shard0 == (63547, 16, 65536, 16, 65536)


def test_scatter_has_thousands_of_short_runs():
    shards, shard0 = _shape("scatter")
    assert shards == [(64513, 16)]
    assert shard0 == (21500, 12284, 32768, 16384, 65536)
    mem = _run("scatter")[1].mem[0]
    assert (mem[:, 1] >> 27 & 1).sum() == 4300 and not np.array_equal(np.argsort(mem[:, 1], kind="stable"), np.arange(len(mem)))


def test_big_read_reaches_twice_the_cpu_table():
    shards, shard0 = _shape("read16000")
    assert shards == [(8, 13)]
    assert shard0 == (16000, 16000, 16384, 16384, 8192)


def test_big_read_meets_the_cap_exactly():
    shards, shard0 = _shape("read16384")
    assert shards == [(7, 13)]
    assert shard0 == (16384, 16384, 16384, 16384, 8192)
    canon = _run("read16384")[3]
    assert canon[7][:, rv32mem.G_MULT].all() and canon[8][:, rv32mem.B_REAL].all()      # no padding row in either table


def test_scatter_of_1024_blocks_exactly():
    shards, shard0 = _shape("blocks1024")
    assert shards == [(130518, 17)]
    assert shard0[0] == 131072 == 1024 * 128 and shard0[2] == 131072 and shard0[4] == 131072


def test_scatter_of_1025_blocks_doubles_memop():
    shards, shard0 = _shape("blocks1025")
    assert shards == [(130518, 17)]
    assert shard0 == (131073, 111317, 262144, 131072, 131072) and -(-shard0[0] // 128) == 1025


@pytest.fixture(scope="module")
def mem_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_rv32_scale") / "libemul_rv32_mem.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", "emul_rv32_mem.cpp")], check=True, capture_output=True)
    return C.CDLL(so)


@pytest.mark.parametrize("name", ["scatter", "read16000"])
def test_numpy_witness_balances_and_equals_the_lane_bodies(name, mem_lib):
    """the reference of the GPU tests at their own shapes: every bus of the numpy tables balances (as
    tests/test_rv32_mem_chips.py holds its guests), and emul_rv32mem_shard writes the cpu, memop and memory tables word
    for word"""
    _elf, ex, image, canon = _run(name)
    airs, preps = rv32mem.airs(), rv32mem.preps_of(image)
    joined = [c if pm is None else np.concatenate([c, pm], axis=1) for c, pm in zip(canon, preps)]
    bal = rv32mem.bus_balance(joined, airs)
    assert set(bal) == {rv32.BUS_PROGRAM, rv32.BUS_RANGE16, rv32.BUS_REGISTER, rv32.BUS_BYTE, rv32cf.BUS_SHIFT, rv32im.BUS_MULDIV,
                        rv32mem.BUS_MEMOP, rv32mem.BUS_MEMORY}
    assert all(v == {} for v in bal.values()), {b: len(v) for b, v in bal.items()}
    s, (_c, data), (start, _end, ecalls), mem = ex.segments[0], ex.witness[0], ex.rv32[0], ex.mem[0]
    tr = rv32.trace_of(s, data)[0]
    ptr = lambda a: a.ctypes.data_as(_lib.u32p)
    rows = np.ascontiguousarray(np.stack([tr[c] for c in ("pc", "ins", "a", "b", "res", "next", "wr")], axis=1), dtype=np.uint32)
    out = [np.full(canon[i].shape, 0xDEADBEEF, dtype=np.uint32) for i in (0, 7, 8)]
    ec = np.ascontiguousarray(ecalls, dtype=np.uint32)
    acc = np.ascontiguousarray(mem, dtype=np.uint32)
    rc = mem_lib.emul_rv32mem_shard(ptr(rows), C.c_size_t(rows.shape[0]), C.c_size_t(canon[0].shape[0]), C.c_uint32(s.end_pc),
                                    ptr(np.ascontiguousarray(start, dtype=np.uint32)), ptr(ec), C.c_size_t(ec.shape[0]), ptr(acc),
                                    C.c_size_t(acc.shape[0]), ptr(out[0]), ptr(out[1]), C.c_size_t(out[1].shape[0]), ptr(out[2]),
                                    C.c_size_t(out[2].shape[0]))
    assert rc == 0
    for g, i in zip(out, (0, 7, 8)):
        assert np.array_equal(g, p3.to_mont(canon[i])), i


def _censuses(tail_spin, po2):
    ex = X.execute(SP.gap_program(SP.GAPS, tail_spin), GAP_INPUT, segment_limit_po2=po2, record_trace=True)
    out = []
    for s, (_c, data), (start, end, ecalls) in zip(ex.segments, ex.witness, ex.rv32):
        cpu = rv32.shard_tables(s, data, start, end, ecalls)[0][0]
        out.append(SP.census(cpu, 1 << s.po2))
    return [s.cycles for s in ex.segments], out


def test_gaps_reach_every_class_a_two_block_chunk_allows():
    """2^13 rows are 64 blocks, a chunk is two: `earlier block, same chunk` cannot occur, every other class does; the
    second shard starts from registers the first left (timestamp 0)"""
    cycles, got = _censuses(3000, 13)
    assert cycles == [8192, 5302]
    assert got[0]["earlier block, same chunk"] == 0
    assert all(got[0][c] > 0 for c in SP.CLASSES if c != "earlier block, same chunk"), got[0]
    assert got[1]["init"] > 0


def test_gaps_reach_all_eight_classes_at_2_16():
    cycles, got = _censuses(34000, 16)
    assert cycles[0] == 65536
    assert all(got[0][c] > 0 for c in SP.CLASSES), got[0]


def test_census_classes():
    """the census on hand-made tables of 4 096 rows (32 blocks, one per chunk) and of 16 384 (four per chunk): row ->
    the timestamp of its write's predecessor"""
    for n, rows, want in ((4096, {5: 0, 6: 3 * 6 + 1, 70: 3 * 6 + 2, 200: 3 * 193 + 1, 300: 3 * 130 + 3, 1000: 3 * 500 + 1},
                           {"init": 1, "same row": 1, "same block": 1, "same wave": 1, "previous block": 1, "earlier chunk": 1}),
                          (16384, {500: 3 * 10 + 1, 600: 3 * 300 + 2, 1400: 3 * 10 + 1},
                           {"earlier block, same chunk": 1, "previous chunk": 1, "earlier chunk": 1})):
        cpu = np.zeros((n, rv32.CPU_COLS), dtype=np.int64)
        for r, pts in rows.items():
            cpu[r, rv32.ACTIVE], cpu[r, rv32.WR], cpu[r, rv32.PW_TS] = 1, 1, pts
            cpu[r, rv32.PA_TS] = cpu[r, rv32.PB_TS] = 3 * r + 1                  # both reads: the row itself
        got = SP.census(cpu, n)
        assert got.pop("same row") == 2 * len(rows) + want.pop("same row", 0)
        assert {k: v for k, v in got.items() if v} == want
