"""The rv32im-elf chip set on the CPU (raiko_amd/rv32elf.py): the program image against the C loader's
(rk_exec_program_image), the preprocessed matrices against the full-width rows rv32im's AIRs prove consistent, every AIR
satisfied and every bus balanced over [trace | preprocessed] on honest shards, the lane bodies of rv32_rows.hpp against
numpy word for word, forgeries refused by the one constraint or the PROGRAM bus, a guest that rewrites its own code
accepted by rv32im and refused here, and the image lister run on hostile headers under sanitizers as a program of its
own."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import rv32_asm as A
import rv32_cf_programs as CP
import rv32_chip_programs as RP
import rv32_elf_programs as EP
import rv32_m_programs as MP
from raiko_amd import _lib, p3, rv32, rv32cf, rv32elf, rv32im
from raiko_amd import executor as X

INPUT = [11, 22, 33, 44]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

IMAGES = {"code": EP.code_only_program, "code+data": lambda: MP.m_program(1), "pow2": EP.pow2_program,
          "one": EP.one_instruction_program, "second": EP.second_segment_program, "sixteen": lambda: EP.SIXTEEN}


def _joined(canon, preps):
    return [c if pm is None else np.concatenate([c, pm], axis=1) for c, pm in zip(canon, preps)]


def test_chip_set_is_registered():
    airs = X._rv32_airs_of("rv32im-elf")
    assert "rv32im-elf" in X.CHIPS and "rv32im-elf" in X.RV32_CHIPS
    assert [a.width for a in airs] == [rv32im.CPU_COLS, 1, rv32.REG_COLS, 1, 1, 1, rv32im.MD_COLS]
    assert [a.prep_width for a in airs] == [0, 42, 0, 4, 1, 4, 0]
    for a in airs:
        assert a.log_quotient_degree() <= 1
        a.handle()
    # the one constraint of the program table; the other lookup tables have none of their own
    assert sum(1 for st in rv32elf.program_air().steps.tolist() if st[0] == p3.ASSERT_ZERO) - \
        sum(1 for st in rv32elf.byte_air().steps.tolist() if st[0] == p3.ASSERT_ZERO) == 1
    # the existing sets are untouched
    assert [a.width for a in X.p3_rv32im_airs()] == [rv32im.CPU_COLS, rv32im.PROGRAM_COLS, rv32.REG_COLS, rv32.BYTE_COLS, 2,
                                                     rv32cf.SHIFT_COLS, rv32im.MD_COLS]


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_program_image_is_the_loaders(name):
    elf = IMAGES[name]()
    image = rv32elf.program_image(elf)
    vaddr, count, words = X.program_image_c(elf)
    assert [v for v, _w in image] == vaddr.tolist() and [w.size for _v, w in image] == count.tolist()
    assert np.array_equal(np.concatenate([w for _v, w in image]), words)
    _pcs, _words, n_rows = rv32elf.image_rows(image)
    assert n_rows >= max(2, words.size) and n_rows & (n_rows - 1) == 0 and (n_rows == 2 or n_rows // 2 < words.size)
    assert n_rows == {"code+data": 1024, "pow2": 64, "one": 2, "sixteen": 16}.get(name, n_rows)
    if name == "code+data":
        assert len(image) == 2 and image[1][0] == 0x00300000
    if name == "pow2":
        assert words.size == n_rows
    # the executor loads the same words
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True) if name != "sixteen" else None
    if ex is not None:
        tr = rv32.trace_of(ex.segments[0], ex.witness[0][1])[0]
        rv32elf.program_mult(tr["pc"], tr["ins"], image)


@pytest.mark.parametrize("name", sorted(EP.HOSTILE))
def test_hostile_images_are_refused_by_both(name):
    elf = EP.HOSTILE[name]
    with pytest.raises(ValueError):
        rv32elf.program_image(elf)
    with pytest.raises(_lib.RkError) as e:
        X.program_image_c(elf)
    assert e.value.status == _lib.RK_ERR_INVALID


def test_seventeen_segments_are_refused_by_both():
    with pytest.raises(ValueError):
        rv32elf.program_image(EP.TOO_MANY)
    with pytest.raises(_lib.RkError) as e:
        X.program_image_c(EP.TOO_MANY)
    assert e.value.status == _lib.RK_ERR_CAPACITY
    assert len(rv32elf.program_image(EP.SIXTEEN)) == 16


def test_image_capacity_protocol():
    lib = _lib.load()
    elf = MP.m_program(1)
    n_segs, n_words = C.c_size_t(0), C.c_size_t(0)
    vaddr, count, words = (np.full(k, 0xDEADBEEF, dtype=np.uint32) for k in (2, 2, 10))
    st = lib.rk_exec_program_image(elf, len(elf), vaddr.ctypes.data_as(_lib.u32p), count.ctypes.data_as(_lib.u32p), 2, C.byref(n_segs),
                                   words.ctypes.data_as(_lib.u32p), 10, C.byref(n_words))
    assert st == _lib.RK_ERR_CAPACITY and (n_segs.value, n_words.value) == (2, 954)
    assert (vaddr == 0xDEADBEEF).all() and (words == 0xDEADBEEF).all()


@pytest.fixture(scope="module")
def full_rows():
    image = rv32elf.program_image(EP.second_segment_program())
    return image, rv32elf.program_full_rows(image), rv32.byte_rows(), rv32cf.shift_rows()


def test_prep_tables_are_the_tuple_columns_of_the_proven_rows(full_rows):
    image, full, byt, sh = full_rows
    prog, pbyte, prange, pshift = rv32elf.prep_tables(image)
    tuple_cols = list(range(20)) + list(range(77, 89)) + list(range(89, 98))
    assert rv32elf.TUPLE_COLS == tuple_cols and prog.shape == (16, 42)
    assert np.array_equal(prog[:, :41], full[:, tuple_cols])
    assert np.array_equal(pbyte, byt[:, [rv32.Y_OP, rv32.Y_X, rv32.Y_Y, rv32.Y_Z]]) and pbyte.shape == (1 << 18, 4)
    assert np.array_equal(pshift, sh[:, [rv32cf.H_K, rv32cf.H_X, rv32cf.H_LO, rv32cf.H_HI]]) and pshift.shape == (1 << 12, 4)
    assert np.array_equal(prange[:, 0], np.arange(1 << 16))
    # the tuple order is the cpu row's: column c of the program tuple is what cpu column PROGRAM_TUPLE[c] sends
    im_air = rv32im.program_air()
    recv = [it for it in im_air.interactions if it.bus == rv32.BUS_PROGRAM][0]
    assert list(recv.value_cols) == tuple_cols
    # VALID: the opcode-class sum, except OP words with bit 25 set that are no M word; padding rows (word 0) are 0
    n = sum(w.size for _v, w in image)
    assert prog[:n, 41].all() and not prog[n:, 41].any()
    odd = np.array([0x02000033, 0x42000033, 0x0200_0033 | 1 << 26, 0x00000033, 0xFFFFFFFF, 0x00000000, 0x00000073], dtype=np.int64)
    f = rv32elf.program_full_rows([(0x1000, odd)])
    assert rv32elf.valid_of(f)[:7].tolist() == [1, 0, 0, 1, 0, 0, 1]


def test_full_rows_pass_the_existing_airs(full_rows):
    """the reference of the preprocessed matrices: rows the rv32im program / byte / shift AIRs accept.  The program and
    shift rows are checked in full.  The byte table is a SAMPLE, as in tests/test_rv32_chips.py: about 1 000 single-row
    slices of its 2^18 rows (every 251st used row, every 4099th padding row, the first and last row of every op) -- the
    byte AIR has no constraint across rows, so a row is judged alone; a full pass costs minutes in check_trace"""
    _image, full, byt, sh = full_rows
    assert rv32im.program_air().check_trace(full) == []
    assert rv32cf.shift_air().check_trace(sh) == []
    rows = np.concatenate([np.arange(0, 3 << 16, 251), np.arange(3 << 16, 1 << 18, 4099),
                           [0, 255, 65535, 65536, 131071, 131072, 196607]])
    bair = rv32.byte_air()
    for r in rows.tolist():
        assert bair.check_trace(byt[r:r + 1]) == [], r


RUNS = {"m25": lambda: MP.m_program(25), "mixed400": lambda: MP.mixed_program(400), "cf1": lambda: CP.cf_program(1),
        "second": EP.second_segment_program, "pow2": EP.pow2_program}
_runs = {}


def _run(name):
    if name not in _runs:
        elf = RUNS[name]()
        ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
        image = rv32elf.program_image(elf)
        _runs[name] = (elf, ex, image, rv32elf.preps_of(image))
    return _runs[name]


@pytest.fixture(scope="module")
def elf_airs():
    return rv32elf.airs()


@pytest.mark.parametrize("name", ["m25", "mixed400", "cf1"])
def test_honest_shards_satisfy_every_air_and_bus(name, elf_airs):
    _elf, ex, image, preps = _run(name)
    assert len(ex.segments) >= (3 if name != "cf1" else 1) and ex.segments[-1].cycles < 1 << 13
    ref = X.p3_rv32im_shards(ex) if name == "cf1" else None
    for k, (s, (_code, data), (start, end, ecalls)) in enumerate(zip(ex.segments, ex.witness, ex.rv32)):
        canon, pub_cpu, pub_reg = rv32elf.shard_tables(s, data, start, end, ecalls, image)
        bal = rv32.bus_balance(_joined(canon, preps), elf_airs)
        assert set(bal) == {rv32.BUS_PROGRAM, rv32.BUS_RANGE16, rv32.BUS_REGISTER, rv32.BUS_BYTE, rv32cf.BUS_SHIFT,
                            rv32im.BUS_MULDIV}
        assert all(v == {} for v in bal.values()), (k, {b: len(v) for b, v in bal.items()})
        pubs = [pub_cpu, (), pub_reg, (), (), (), ()]
        # byte, range and shift have no constraint of their own, only the receive the bus balance above covers: they go
        # through check_trace for shard 0 only (a pass over 2^18 rows that can refuse nothing)
        for i in (0, 1, 6) if k else range(7):
            assert elf_airs[i].check_trace(canon[i], pubs[i], prep=preps[i]) == [], (k, i)
        assert canon[1].sum() == s.cycles and canon[1].shape == (preps[1].shape[0], 1)
        if ref is not None:                             # cpu, register and muldiv are rv32im's, the counts its histograms
            want = RP.tables_canon(ref[k][0])
            for i in (0, 2, 6):
                assert np.array_equal(canon[i], want[i])
            assert np.array_equal(canon[3][:, 0], want[3][:, rv32.Y_MULT]) and np.array_equal(canon[4][:, 0], want[4][:, 1])
            assert np.array_equal(canon[5][:, 0], want[5][:, rv32cf.H_MULT])
            assert not canon[6][:, rv32im.D_MULT].any()


@pytest.fixture(scope="module")
def elf_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_rv32_elf") / "libemul_rv32_elf.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", "emul_rv32_elf.cpp")], check=True, capture_output=True)
    return C.CDLL(so)


@pytest.mark.parametrize("name", ["second", "pow2", "mixed400"])
def test_lane_bodies_write_the_numpy_tables(elf_lib, name):
    """tests/emul/emul_rv32_elf.cpp: the preprocessed matrices and the program count column through rv32_rows.hpp's
    bodies are rv32elf.prep_tables / shard_tables word for word in Montgomery form; `second` runs code in the second
    executable segment, whose rows start after the first one's"""
    elf, ex, image, preps = _run(name)
    vaddr, count, words = X.program_image_c(elf)
    ptr = lambda a: a.ctypes.data_as(_lib.u32p)
    want = [p3.to_mont(preps[i]) for i in (1, 3, 4, 5)]
    got = [np.full(w.shape, 0xDEADBEEF, dtype=np.uint32) for w in want]
    rc = elf_lib.emul_rv32elf_prep(ptr(vaddr), ptr(count), C.c_uint32(vaddr.size), ptr(words), C.c_size_t(words.size), ptr(got[0]),
                                   C.c_size_t(want[0].shape[0]), ptr(got[1]), ptr(got[2]), ptr(got[3]))
    assert rc == 0
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    ran_second = False
    for s, (_code, data), (start, end, ecalls) in zip(ex.segments, ex.witness, ex.rv32):
        canon = rv32elf.shard_tables(s, data, start, end, ecalls, image)[0]
        tr = rv32.trace_of(s, data)[0]
        rows = np.ascontiguousarray(np.stack([tr[k] for k in ("pc", "ins", "a", "b", "res", "next", "wr")], axis=1), dtype=np.uint32)
        mult = np.full(canon[1].shape[0], 0xDEADBEEF, dtype=np.uint32)
        rc = elf_lib.emul_rv32elf_program_mult(ptr(vaddr), ptr(count), C.c_uint32(vaddr.size), ptr(words), C.c_size_t(words.size),
                                               ptr(rows), C.c_size_t(rows.shape[0]), ptr(mult), C.c_size_t(mult.size))
        assert rc == 0 and np.array_equal(mult, p3.to_mont(canon[1][:, 0]))
        ran_second |= bool(len(image) > 1 and canon[1][image[0][1].size:, 0].any())
    assert ran_second == (name == "second")


def test_forgeries_are_refused(elf_airs):
    _elf, ex, image, preps = _run("second")
    s, (_code, data), (start, end, ecalls) = ex.segments[0], ex.witness[0], ex.rv32[0]
    canon = rv32elf.shard_tables(s, data, start, end, ecalls, image)[0]
    # multiplicity 1 on a padding row (VALID = 0): the one constraint
    t = canon[1].copy()
    pad = preps[1].shape[0] - 1
    assert preps[1][pad, rv32elf.P_VALID] == 0
    t[pad, 0] = 1
    assert elf_airs[1].check_trace(t, (), prep=preps[1]) == [(pad, 0)]
    assert elf_airs[1].check_trace(canon[1], (), prep=preps[1]) == []
    # a cpu row whose looked-up tuple differs from the image row in one field: the PROGRAM bus
    for col in (rv32.IMM_LO, rv32.RS1, rv32im.IS_MUL, rv32.INS_LO):
        cpu = canon[0].copy()
        cpu[1, col] ^= 1
        forged = [cpu] + canon[1:]
        bal = rv32.bus_balance(_joined(forged, preps), elf_airs)
        assert bal[rv32.BUS_PROGRAM], col
    assert all(v == {} for v in rv32.bus_balance(_joined(canon, preps), elf_airs).values())


def test_self_modifying_guest_is_the_gap_and_is_closed():
    elf = EP.selfmod_program()
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    s, (_code, data), (start, end, ecalls) = ex.segments[0], ex.witness[0], ex.rv32[0]
    tr = rv32.trace_of(s, data)[0]
    new = A.encode("addi", ("a2", "zero", 2), 0, {})
    at = tr["pc"].tolist().index(EP.BASE + 20)
    assert tr["ins"][at] == new and end[A.REG["a3"]] == 4          # the rewritten instruction ran
    canon = rv32im.shard_tables(s, data, start, end, ecalls)[0]    # rv32im proves it without complaint
    airs = rv32im.airs()
    assert all(v == {} for v in rv32.bus_balance(canon, airs).values()) and airs[1].check_trace(canon[1]) == []
    image = rv32elf.program_image(elf)
    assert image[0][1][5] != new
    with pytest.raises(ValueError, match="not the program image's word"):
        rv32elf.shard_tables(s, data, start, end, ecalls, image)
    # a pc outside every executable segment
    with pytest.raises(ValueError, match="outside the program image"):
        rv32elf.program_mult(np.array([0x00400000]), np.array([0x13]), image)
    with pytest.raises(ValueError, match="outside the program image"):
        rv32elf.program_mult(np.array([EP.BASE + 2]), np.array([0x13]), image)


def test_image_lister_on_hostile_headers_under_sanitizers(tmp_path):
    """tests/asan/elf_image_main.cpp: a program of its own (nothing is loaded into Python), built from
    raiko_amd/csrc/elf_image.cpp with -fsanitize=address,undefined: truncations at every length, filesz > memsz, offsets
    past the end, phnum 0, 17 executable segments, byte mutations of the headers, undersized output buffers"""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = str(tmp_path / "elf_image_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "asan", "elf_image_main.cpp"), os.path.join(ROOT, "raiko_amd", "csrc", "elf_image.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "elf_image_main ok" in r.stdout
