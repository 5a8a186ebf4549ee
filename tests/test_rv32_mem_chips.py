"""The rv32im-mem chip set on the CPU (raiko_amd/rv32mem.py): the executor's access list against a plain-Python replay of
the guest, the preprocessed program matrix, every AIR satisfied and every bus balanced on honest shards, the lane bodies
of rv32_rows.hpp against numpy word for word, and forged witnesses refused each by a named constraint or a bus -- the
forged load among them verifies under rv32im-elf, which is what the chip set is for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rv32_asm as A
import rv32_mem_programs as GP
from raiko_amd import _lib, p3, rv32, rv32cf, rv32elf, rv32im, rv32mem
from raiko_amd import executor as X
from raiko_amd.segment import P

INPUT = [0x11223344, 0x80FF7F01, 0xDEADBEEF, 0x00000044]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = dict(GP.GUESTS, two=GP.two_shard_program, forge=GP.forge_program, one_word=lambda: GP.count_program(129),
            distinct=lambda: GP.count_program(129, distinct=True), none=lambda: GP.count_program(0))
_runs = {}


def _run(name):
    if name not in _runs:
        elf = RUNS[name]()
        ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
        image = rv32elf.program_image(elf)
        _runs[name] = (elf, ex, image, rv32mem.preps_of(image))
    return _runs[name]


def _shards(ex):
    return zip(ex.segments, ex.witness, ex.rv32, ex.mem)


def _joined(canon, preps):
    return [c if pm is None else np.concatenate([c, pm], axis=1) for c, pm in zip(canon, preps)]


@pytest.fixture(scope="module")
def airs():
    return rv32mem.airs()


def _named(air, bad):
    """check_trace's (row, constraint index) -> {(row, constraint name)}"""
    back = {v: k for k, v in air.constraint_names.items()}
    return {(r, back.get(k, k)) for r, k in bad}


def _first_row_only(air, k):
    """constraint k of the cpu AIR is one of those under when_first_row (the public pc and TSA = 1)"""
    if not hasattr(air, "_first_only"):
        t = np.zeros((2, air.width), dtype=np.int64)
        t[:, rv32.TSA] = [1, 4]
        base = {kk for r, kk in air.check_trace(t, [0, 0, 0, 0]) if r == 0}
        t[0, rv32.TSA], t[0, rv32.PC_LO], t[0, rv32.PC_HI] = 7, 5, 6
        air._first_only = {kk for r, kk in air.check_trace(t, [0, 0, 0, 0]) if r == 0} - base
    return k in air._first_only


def _check(airs, canon, preps, pubs, cpu_rows=None):
    """every AIR on every row (the cpu table on its first cpu_rows rows and its last: padding rows repeat) -> named
    failures per table; the byte, range and shift tables have no constraints"""
    out = {}
    for i in (0, 1, 2, 6, 7, 8):
        t, pm = canon[i], preps[i]
        if i == 0 and cpu_rows is not None:                # rows cpu_rows.. are identical padding rows but for TSA
            # a slice's last row wraps to its first: not judged.  A long shard (the spin loop of `two`) is judged on its
            # first and last 300 cycles, where its memory rows are; the loop between repeats three rows
            cuts = [(0, cpu_rows + 2)] if cpu_rows <= 600 else [(0, 301), (cpu_rows - 300, cpu_rows + 2)]
            bad = []
            for lo, hi in cuts:
                pv = list(pubs[0])
                if lo:                                      # the first-row constraints bind row 0 of the table only
                    pv[0], pv[1] = t[lo, rv32.PC_LO], t[lo, rv32.PC_HI]
                got = airs[0].check_trace(t[lo:hi], pv)
                first = {k for r, k in got if r == 0} if lo else set()
                bad += [(r + lo, k) for r, k in got if r != hi - lo - 1 and not (lo and r == 0 and k in first and _first_row_only(airs[0], k))]
        else:
            bad = airs[i].check_trace(t, pubs[i], prep=pm)
        if bad:
            out[i] = _named(airs[i], bad) if hasattr(airs[i], "constraint_names") else bad
    return out


def test_chip_set_is_registered(airs):
    assert "rv32im-mem" in X.CHIPS and "rv32im-mem" in X.RV32_CHIPS and X.KEYED_CHIPS == ("rv32im-elf", "rv32im-mem")
    got = X._rv32_airs_of("rv32im-mem")
    assert [a.width for a in got] == [141, 1, rv32.REG_COLS, 1, 1, 1, rv32im.MD_COLS, 64, 13]
    assert [a.prep_width for a in got] == [0, 48, 0, 4, 1, 4, 0, 0, 0]
    assert rv32mem.CPU_COLS == rv32im.CPU_COLS + 9 and rv32mem.PROGRAM_TUPLE[:41] == rv32im.PROGRAM_TUPLE
    for a in got:
        assert a.log_quotient_degree() <= 1                 # every constraint has degree <= 3
        a.handle()                                          # the library takes the step list and the interactions
    # the existing sets are untouched
    assert [a.width for a in X._rv32_airs_of("rv32im-elf")] == [rv32im.CPU_COLS, 1, rv32.REG_COLS, 1, 1, 1, rv32im.MD_COLS]
    assert [a.prep_width for a in X._rv32_airs_of("rv32im-elf")] == [0, 42, 0, 4, 1, 4, 0]


def test_program_key_fields():
    elf, _ex, image, preps = _run("ops")
    prog = preps[1]
    old = rv32elf.prep_tables(image)[0]
    assert prog.shape == (old.shape[0], 48) and np.array_equal(prog[:, :41], old[:, :41])
    lw = A.encode("lw", ("a2", -4, "s0"), 0, {})
    sh = A.encode("sh", ("t1", -2, "s1"), 0, {})
    sb = A.encode("sb", ("t1", 0x7FF, "s1"), 0, {})
    odd = np.array([lw, sh, sb, 0x73, lw | 3 << 12, lw | 6 << 12, lw | 7 << 12, sh | 3 << 12, sh | 4 << 12, 0x13], dtype=np.int64)
    fields, ok = rv32mem.decode(odd)
    assert fields[:4].tolist() == [[1, 0, 2, 0xFFFC, 0xFFFF, 0], [0, 1, 9, 0xFFFE, 0xFFFF, 0], [0, 1, 8, 0x7FF, 0, 0],
                                   [0, 0, 0, 0, 0, 1]]
    assert ok.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 1]
    f = rv32mem.prep_tables([(0x1000, odd)])[0]
    assert f[:10, 47].tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0, 1] and not f[10:, 47].any()
    n = sum(w.size for _v, w in image)
    assert prog[:n - 4, 47].all()                           # the guest's code words; the four data words are no instructions


@pytest.mark.parametrize("name", sorted(RUNS))
def test_access_list_is_the_replay(name):
    elf, ex, _image, _preps = _run(name)
    memory, pos, total = None, 0, 0
    for s, (_code, data), (start, _end, ecalls), mem in _shards(ex):
        tr = rv32.trace_of(s, data)[0]
        want, memory, pos = GP.replay(elf, tr, start, ecalls, INPUT, memory, pos)
        assert [tuple(r) for r in mem.tolist()] == want
        total += len(want)
    assert total == {"one_word": 129, "distinct": 129, "none": 0, "x0": 3, "two": 6}.get(name, total)
    if name == "ecall":                                     # three words at the first ecall's cycle, one at the second's
        mem = ex.mem[0]
        first, second = ex.rv32[0][2][:2, 0].tolist()       # the cycles of the two READ ecalls
        assert (mem[:, 0] == first).sum() == 3 and (mem[:, 0] == second).sum() == 1
        assert mem[mem[:, 0] == first, 3].tolist() == INPUT[:3] and mem[mem[:, 0] == second, 3].tolist() == INPUT[3:4]
        assert mem[mem[:, 0] == first, 1].tolist() == [(GP.DATA + 0x40 + 4 * k) >> 2 for k in range(3)]


@pytest.fixture(scope="module")
def mem_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_rv32_mem") / "libemul_rv32_mem.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", "emul_rv32_mem.cpp")], check=True, capture_output=True)
    return C.CDLL(so)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_honest_shards_satisfy_every_air_and_bus_and_the_lane_bodies_write_them(name, airs, mem_lib):
    """the numpy witness satisfies all nine AIRs and every bus balances; tests/emul/emul_rv32_mem.cpp walks the lane
    bodies of rv32_rows.hpp over the same trace and access list and matches numpy word for word"""
    elf, ex, image, preps = _run(name)
    ptr = lambda a: a.ctypes.data_as(_lib.u32p)
    vaddr, count, words = X.program_image_c(elf)
    got = np.full(preps[1].shape, 0xDEADBEEF, dtype=np.uint32)
    assert mem_lib.emul_rv32mem_prep(ptr(vaddr), ptr(count), C.c_uint32(vaddr.size), ptr(words), C.c_size_t(words.size), ptr(got),
                                     C.c_size_t(got.shape[0])) == 0
    assert np.array_equal(got, p3.to_mont(preps[1]))
    assert len(ex.segments) == (2 if name == "two" else 1)
    for k, (s, (_code, data), (start, end, ecalls), mem) in enumerate(_shards(ex)):
        canon, pub_cpu, pub_reg = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)
        bal = rv32mem.bus_balance(_joined(canon, preps), airs)
        assert set(bal) == {rv32.BUS_PROGRAM, rv32.BUS_RANGE16, rv32.BUS_REGISTER, rv32.BUS_BYTE, rv32cf.BUS_SHIFT, rv32im.BUS_MULDIV,
                            rv32mem.BUS_MEMOP, rv32mem.BUS_MEMORY}
        assert all(v == {} for v in bal.values()), (k, {b: len(v) for b, v in bal.items()})
        pubs = [pub_cpu, (), pub_reg] + [()] * 6
        assert _check(airs, canon, preps, pubs, cpu_rows=s.cycles) == {}
        # heights: 2^max(1, ceil(log2 count))
        n_words = np.unique(mem[:, 1]).size
        assert canon[7].shape[0] == max(2, 1 << int(len(mem) - 1).bit_length() if len(mem) else 2)
        assert canon[8].shape[0] == max(2, 1 << int(n_words - 1).bit_length() if n_words else 2)
        assert canon[7][:, rv32mem.G_MULT].sum() == len(mem) and canon[8][:, rv32mem.B_REAL].sum() == n_words
        assert canon[0][:, rv32mem.M_MEM].sum() + canon[0][:, rv32mem.N_ECW].sum() == len(mem)
        # the lane bodies
        tr = rv32.trace_of(s, data)[0]
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
    if name == "one_word":
        assert canon[8].shape[0] == 2 and canon[7].shape[0] == 256 and canon[7][128, rv32mem.G_PTS] == canon[7][127, rv32mem.G_TS]
    if name == "distinct":
        assert canon[8].shape[0] == canon[7].shape[0] == 256 and not canon[7][:, rv32mem.G_PTS].any()
    if name == "none":
        assert canon[7].shape[0] == canon[8].shape[0] == 2 and not canon[7][:, :rv32mem.G_ONE].any()


def test_ops_cover_every_case():
    """the `ops`, `far`, `wrap` and `x0` guests hold the cases the chip set is tested on"""
    _elf, ex, image, _preps = _run("ops")
    s, (_c, data), (start, end, ecalls), mem = next(_shards(ex))
    mo = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)[0][7]
    on = mo[mo[:, rv32mem.G_MULT] == 1]
    off = on[:, rv32mem.G_O0] + 2 * on[:, rv32mem.G_O1]
    sel = on[:, :9].argmax(axis=1)
    seen = {(rv32mem.OPS[k], int(o)) for k, o in zip(sel, off)}
    want = {(op, o) for op in ("lb", "lbu", "sb") for o in range(4)} | {(op, o) for op in ("lh", "lhu", "sh") for o in (0, 2)} | \
        {("lw", 0), ("sw", 0)}
    assert seen == want
    res = on[:, rv32mem.G_R_LO] | on[:, rv32mem.G_R_HI] << 16
    lb, lh = res[sel == 0].tolist(), res[sel == 1].tolist()
    assert 0x7F in lb and 0xFFFFFF80 in lb and 0x7FFF in lh and 0xFFFF8000 in lh
    assert 0x80 in res[sel == 3].tolist() and 0x8000 in res[sel == 4].tolist()
    # far: word addresses that differ only in WH bits; wrap: a carry out of the address sum; x0: loads that send nothing
    _elf, ex, image, _preps = _run("far")
    bd = rv32mem.memory_rows(ex.mem[0])[0]
    assert len(set(bd[:4, rv32mem.B_WL].tolist())) == 1 and len(set(bd[:4, rv32mem.B_WH].tolist())) == 4
    _elf, ex, image, _preps = _run("wrap")
    s, (_c, data), (start, end, ecalls), mem = next(_shards(ex))
    mo = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)[0][7]
    assert mo[0, rv32mem.G_K1] == 1 and mo[0, rv32mem.G_AD_LO] == 4 and mo[0, rv32mem.G_AD_HI] == 0
    _elf, ex, image, _preps = _run("x0")
    s, (_c, data), (start, end, ecalls), mem = next(_shards(ex))
    cpu = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)[0][0]
    assert cpu[:, rv32mem.IS_LOAD].sum() == 6 and cpu[:, rv32mem.M_MEM].sum() == 3 == len(mem)


def test_two_shards_chain_and_the_boundary_is_free(airs):
    """the second shard loads what the first stored: the run verifies as a chain of registers and pcs.  Its memory is NOT
    chained: INIT of a touched word is free, so a second shard that starts the word from another value -- and loads that
    value -- satisfies every AIR and bus as well.  Binding INIT to the previous shard's FINAL is the follow-up"""
    _elf, ex, image, preps = _run("two")
    pubs, tables = [], []
    for s, (_c, data), (start, end, ecalls), mem in _shards(ex):
        canon, pc, pr = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)
        pubs.append((pc, pr))
        tables.append(canon)
    assert X.check_rv32_chain(pubs, entry_pc=ex.segments[0].start_pc)
    first, second = tables[0][8], tables[1][8]
    w = (GP.DATA + 8) >> 2
    at = lambda t: t[(t[:, rv32mem.B_WL] | t[:, rv32mem.B_WH] << 14) == w][0]
    assert at(first)[rv32mem.B_F_LO] | at(first)[rv32mem.B_F_HI] << 16 == 0x5EEDBEEF
    assert at(second)[rv32mem.B_I_LO] | at(second)[rv32mem.B_I_HI] << 16 == 0x5EEDBEEF       # the honest prover's INIT
    # another INIT: the load of that word (lw a2: nothing reads a2 afterwards) returns it
    s, (_c, data), (start, _end, ecalls), mem = list(_shards(ex))[1]
    tr = rv32.trace_of(s, data)[0]
    c = tr["ins"].tolist().index(A.encode("lw", ("a2", 8, "s0"), 0, {}))
    data, mem = data.copy(), mem.copy()
    data[rv32.RES_LO, c], data[rv32.RES_HI, c] = p3.to_mont([0x1234, 0x5678])
    k = np.nonzero(mem[:, 0] == c)[0][0]
    mem[k, 2] = mem[k, 3] = 0x56781234
    canon, pc, pr = rv32mem.shard_tables(s, data, start, None, ecalls, image, mem)
    assert all(v == {} for v in rv32mem.bus_balance(_joined(canon, preps), airs).values())
    assert _check(airs, canon, preps, [pc, (), pr] + [()] * 6, cpu_rows=s.cycles) == {}


# ------------------------------------------------------------------------------------------------ forgeries
@pytest.fixture(scope="module")
def honest(airs):
    _elf, ex, image, preps = _run("forge")
    s, (_c, data), (start, end, ecalls), mem = next(_shards(ex))
    canon, pc, pr = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)
    tr = rv32.trace_of(s, data)[0]
    cyc = lambda *ins: tr["ins"].tolist().index(A.encode(ins[0], ins[1:], 0, {}))
    return dict(s=s, data=data, start=start, end=end, ecalls=ecalls, mem=mem, image=image, preps=preps, canon=canon,
                pubs=[pc, (), pr] + [()] * 6, cyc=cyc, row=lambda c: int(np.nonzero(mem[:, 0] == c)[0][0]))


def _forged_res(h, c, value, mem=None):
    data = h["data"].copy()
    data[rv32.RES_LO, c], data[rv32.RES_HI, c] = p3.to_mont([value & 0xFFFF, value >> 16])
    return data, rv32mem.shard_tables(h["s"], data, h["start"], None, h["ecalls"], h["image"], h["mem"] if mem is None else mem)


def test_forged_load_verifies_under_rv32im_elf_and_is_refused_here(airs, honest):
    """lw a5 after sw to the same word claims another value; a5 is never read, so the register file stays consistent"""
    h = honest
    c = h["cyc"]("lw", "a5", 8, "s0")
    data, (canon, pc, pr) = _forged_res(h, c, 0x0BAD0BAD)
    # rv32im-elf: every AIR holds and every bus balances -- the load's result is a free cell there
    elf_airs, elf_preps = rv32elf.airs(), rv32elf.preps_of(h["image"])
    ecanon, epc, epr = rv32elf.shard_tables(h["s"], data, h["start"], None, h["ecalls"], h["image"])
    assert ecanon[0][c, rv32.RES_LO] == 0x0BAD and ecanon[2][15, rv32.R_FL] == 0x0BAD        # a5 ends with the forged value
    assert all(v == {} for v in rv32.bus_balance(_joined(ecanon, elf_preps), elf_airs).values())
    for i in (0, 1, 2, 6):
        t = ecanon[i][:h["s"].cycles + 2] if i == 0 else ecanon[i]
        bad = [b for b in elf_airs[i].check_trace(t, [epc, (), epr, (), (), (), ()][i], prep=elf_preps[i]) if i or b[0] != h["s"].cycles + 1]
        assert bad == []
    # rv32im-mem: the memop row of that load names the stored word, the claimed result is not it
    k = h["row"](c)
    assert _check(airs, canon, h["preps"], [pc, (), pr] + [()] * 6, cpu_rows=h["s"].cycles) == {7: {(k, "lw lo"), (k, "lw hi")}}
    # a forger who also rewrites the word the load sees satisfies the row and breaks the word's history
    mem = h["mem"].copy()
    mem[k, 2] = mem[k, 3] = 0x0BAD0BAD
    _data, (canon, pc, pr) = _forged_res(h, c, 0x0BAD0BAD, mem)
    assert _check(airs, canon, h["preps"], [pc, (), pr] + [()] * 6, cpu_rows=h["s"].cycles) == {}
    bal = rv32mem.bus_balance(_joined(canon, h["preps"]), airs)
    assert bal[rv32mem.BUS_MEMORY] and all(v == {} for b, v in bal.items() if b != rv32mem.BUS_MEMORY)


def test_forged_sign_extension(airs, honest):
    h = honest
    c = h["cyc"]("lb", "a4", 1, "s0")
    assert h["canon"][0][c, rv32.RES_LO] == 0xFF80 and h["canon"][0][c, rv32.RES_HI] == 0xFFFF
    _data, (canon, pc, pr) = _forged_res(h, c, 0x80)                       # zero-extended
    k = h["row"](c)
    assert _check(airs, canon, h["preps"], [pc, (), pr] + [()] * 6, cpu_rows=h["s"].cycles) == {7: {(k, "lb lo"), (k, "lb hi")}}
    c = h["cyc"]("lh", "a3", 6, "s0")
    _data, (canon, pc, pr) = _forged_res(h, c, 0x00008000)
    assert _check(airs, canon, h["preps"], [pc, (), pr] + [()] * 6, cpu_rows=h["s"].cycles) == {7: {(h["row"](c), "lh hi")}}
    # the sign bit itself is the shift table's: a row that claims SG = 0 for the byte 0x80 finds no tuple there
    t = [x.copy() for x in h["canon"]]
    k = h["row"](h["cyc"]("lb", "a4", 1, "s0"))
    t[7][k, rv32mem.G_SG], t[7][k, rv32mem.G_R_LO], t[7][k, rv32mem.G_R_HI] = 0, 0x80, 0
    t[0][h["cyc"]("lb", "a4", 1, "s0"), rv32.RES_LO], t[0][h["cyc"]("lb", "a4", 1, "s0"), rv32.RES_HI] = 0x80, 0
    assert airs[7].check_trace(t[7]) == []
    assert rv32mem.bus_balance(_joined(t, h["preps"]), airs)[rv32cf.BUS_SHIFT]


def test_forged_store_byte_changes_a_neighbour(airs, honest):
    h = honest
    c = h["cyc"]("sb", "t1", 13, "s0")
    k = h["row"](c)
    mem = h["mem"].copy()
    assert mem[k, 2] == 0 and mem[k, 3] == 0x68 << 8
    mem[k, 3] |= 0x99 << 16                                                 # byte 2 changes as well
    canon, pc, pr = rv32mem.shard_tables(h["s"], h["data"], h["start"], h["end"], h["ecalls"], h["image"], mem)
    assert _check(airs, canon, h["preps"], [pc, (), pr] + [()] * 6, cpu_rows=h["s"].cycles) == {7: {(k, "sb 2")}}


def test_forged_rows_of_memop(airs, honest):
    h = honest
    G = rv32mem
    base = h["canon"][7]
    assert airs[7].check_trace(base) == []
    # a misaligned LH: the address one byte further, the immediate adjusted so that the sum still holds
    k = h["row"](h["cyc"]("lh", "a3", 6, "s0"))
    t = base.copy()
    t[k, G.G_O0], t[k, G.G_AD_LO], t[k, G.G_MI_LO] = 1, t[k, G.G_AD_LO] + 1, t[k, G.G_MI_LO] + 1
    t[k, G.G_S + 2], t[k, G.G_S + 3] = 0, 1
    t[k, G.G_X] = t[k, G.G_W + 3]
    assert _named(airs[7], airs[7].check_trace(t)) == {(k, "align half")}
    # a PTS equal to TS
    k = h["row"](h["cyc"]("lw", "a5", 8, "s0"))
    t = base.copy()
    assert t[k, G.G_PTS] == t[k - 1, G.G_TS] != 0
    t[k, G.G_PTS], t[k, G.G_DL], t[k, G.G_DH] = t[k, G.G_TS], 0, 0
    assert _named(airs[7], airs[7].check_trace(t)) == {(k, "ts")}
    t[k, G.G_DL] = P - 1                                                    # the constraint holds with DL = -1 ...
    assert airs[7].check_trace(t) == []
    canon = list(h["canon"])
    canon[7] = t
    assert rv32mem.bus_balance(_joined(canon, h["preps"]), airs)[rv32.BUS_RANGE16]   # ... which is no 16-bit value
    # a wrong address carry
    t = base.copy()
    t[k, G.G_K0] = 1
    assert _named(airs[7], airs[7].check_trace(t)) == {(k, "addr lo"), (k, "addr hi")}
    # an ECW row at a timestamp that is not an ecall's: no cpu row sends (16, TS) ...
    t = base.copy()
    k = int(base[:, G.G_MULT].sum())                                        # the first padding row
    assert k < t.shape[0] and h["canon"][0][2, rv32mem.IS_SYS] == 0
    t[k, G.G_SEL + 8], t[k, G.G_MULT], t[k, G.G_OP], t[k, G.G_TS], t[k, G.G_S] = 1, 1, 16, 3 * 2 + 1, 1
    t[k, G.G_DL], t[k, G.G_DH] = 6, 0
    assert airs[7].check_trace(t) == []
    canon = list(h["canon"])
    canon[7] = t
    assert (16, 7) in rv32mem.bus_balance(_joined(canon, h["preps"]), airs)[rv32mem.BUS_MEMOP]
    # ... and a cpu row that is no ecall's cannot: N_ECW (1 - IS_SYS) = 0
    cpu = h["canon"][0].copy()
    cpu[2, rv32mem.N_ECW] = 1
    bad = airs[0].check_trace(cpu[:h["s"].cycles + 2], h["pubs"][0])
    assert (2, "n_ecw sys") in _named(airs[0], bad)
    cpu = h["canon"][0].copy()
    cpu[h["s"].cycles + 3, rv32mem.N_ECW], cpu[h["s"].cycles + 3, rv32mem.IS_SYS] = 1, 1      # a padding row
    assert _named(airs[0], airs[0].check_trace(cpu[h["s"].cycles + 3:h["s"].cycles + 4], h["pubs"][0])) >= {(0, "n_ecw padding")}


def test_forged_boundary_rows(airs, honest):
    h = honest
    B = rv32mem
    base = h["canon"][8]
    real = int(base[:, B.B_REAL].sum())
    assert real >= 3 and airs[8].check_trace(base) == []
    bus = lambda t: rv32mem.bus_balance(_joined(h["canon"][:8] + [t], h["preps"]), airs)
    # two rows for one address (two parallel histories): whatever SAME says, a difference is -1 or 0 - 1
    for same in (0, 1):
        t = base.copy()
        t[1] = t[0]
        t[0, B.B_SAME], t[0, B.B_GL], t[0, B.B_GH] = same, 0, 0
        assert (0, "ascending low" if same else "ascending high") in _named(airs[8], airs[8].check_trace(t))
        t[0, B.B_GL if same else B.B_GH] = P - 1                           # the difference itself: no 16-bit limb
        assert not any(r == 0 for r, _k in airs[8].check_trace(t)) and bus(t)[rv32.BUS_RANGE16]
    # rows out of order
    t = base.copy()
    t[[0, 1]] = t[[1, 0]]
    assert {k for r, k in _named(airs[8], airs[8].check_trace(t)) if r == 0} & {"ascending low", "ascending high", "same high"}
    # a real row after a padding row
    t = base.copy()
    t[real - 2] = 0
    assert (real - 2, "padding") in _named(airs[8], airs[8].check_trace(t))


def test_boundary_order_cannot_wrap_the_field(airs):
    """p < 2^31 and word addresses reach 2^30, so ONE comparison of WL + 2^14 WH with a 30-bit gap accepts a negative
    difference as p - d: rows at addresses 100, 10^9, 100 with gaps 999 999 899 and p - 999 999 901, all limbs below
    2^16.  The limb-wise order refuses the step down, whatever the prover writes into SAME, GL and GH"""
    B = rv32mem
    addrs = [100, 1000000000, 100]
    mem = np.array([[k, a, 5, 5] for k, a in enumerate(addrs)], dtype=np.int64)
    assert P - 999999901 == 1013266020 and (1013266020 >> 14) < 1 << 16       # the wrapped gap has legal limbs
    t = np.zeros((4, B.MEMORY_COLS), dtype=np.int64)
    for r, a in enumerate(addrs):
        row = B.memory_rows(mem[r:r + 1])[0][0]
        t[r] = row
        t[r, B.B_FTS], t[r, B.B_FINV] = 3 * r + 1, pow(3 * r + 1, P - 2, P)
    up = B.memory_rows(mem[:2])[0]
    t[0, [B.B_SAME, B.B_GL, B.B_GH]] = up[0, [B.B_SAME, B.B_GL, B.B_GH]]      # 100 -> 10^9: honest
    assert not any(r == 0 for r, _k in airs[8].check_trace(t))
    bad = lambda: {k for r, k in _named(airs[8], airs[8].check_trace(t)) if r == 1}
    wl, wh = 100 & 0x3FFF, 100 >> 14
    nl, nh = 1000000000 & 0x3FFF, 1000000000 >> 14
    for same, gl, gh in ((0, 0, 0), (1, 0, 0), (0, 0, (wh - nh - 1) % P), (1, (wl - nl - 1) % P, 0),
                         (0, 1013266020 & 0x3FFF, 1013266020 >> 14)):
        t[1, [B.B_SAME, B.B_GL, B.B_GH]] = same, gl, gh
        failing = bad()
        limbs_ok = gl < 1 << 16 and gh < 1 << 16
        assert failing & {"ascending low", "ascending high", "same high"} or not limbs_ok, (same, gl, gh)
    # a real row bounds its own address limbs: WL, 4 WL and WH are among what it sends to RANGE16
    sent = {tuple(it.value_cols) for it in airs[8].interactions if it.bus == rv32.BUS_RANGE16}
    assert sent == {(c,) for c in B.MEMORY_RANGE} and {B.B_WL, B.B_WL4, B.B_WH} <= set(B.MEMORY_RANGE)
    t = B.memory_rows(mem[:1])[0]
    t[0, B.B_WL] = 1 << 14                                                    # WL = 2^14: 4 WL is no 16-bit value
    t[0, B.B_WL4] = 1 << 16
    assert airs[8].check_trace(t) == []
    assert (1 << 16,) in rv32mem.bus_balance([t], [airs[8]])[rv32.BUS_RANGE16]   # sent to a table that holds 0 .. 2^16 - 1


def test_untouched_filler_row_is_refused(airs, honest):
    """a real row with F = I and FTS = 0 receives its own send (a tuple is read as padded with zeros): BUS_MEMORY would
    balance with no memop row at all, at any address.  FTS FINV = 1 on real rows forbids it"""
    h = honest
    B = rv32mem
    base = h["canon"][8]
    real = int(base[:, B.B_REAL].sum())
    assert real < base.shape[0]
    t = base.copy()
    last = base[real - 1]
    addr = (last[B.B_WL] | last[B.B_WH] << 14) + 7
    t[real] = 0
    t[real, [B.B_WL, B.B_WH, B.B_WL4, B.B_I_LO, B.B_F_LO, B.B_REAL]] = addr & 0x3FFF, addr >> 14, 4 * (addr & 0x3FFF), 9, 9, 1
    same = int((addr >> 14) == last[B.B_WH])
    t[real - 1, [B.B_SAME, B.B_GL, B.B_GH]] = same, 6 if same else 0, 0 if same else (addr >> 14) - last[B.B_WH] - 1
    bal = rv32mem.bus_balance(_joined(h["canon"][:8] + [t], h["preps"]), airs)
    assert bal[rv32mem.BUS_MEMORY] == {}                                      # the bus alone does not see the row
    assert _named(airs[8], airs[8].check_trace(t)) == {(real, "touched")}
    for finv in (0, 1, P - 1):
        t[real, B.B_FINV] = finv
        assert (real, "touched") in _named(airs[8], airs[8].check_trace(t))


# ------------------------------------------------------------------------------------------------ refusals on the host
def test_access_list_check(mem_lib):
    """rv32_rows.hpp mem_list_ok, what rk_exec_rv32mem_shard_device runs before any launch: the executor's list passes;
    a shuffled, a duplicated, a truncated list, an entry at an ALU row and an address past 2^30 are refused"""
    _elf, ex, _image, _preps = _run("ecall")
    s, (_c, data), _regs, mem = next(_shards(ex))
    tr = rv32.trace_of(s, data)[0]
    rows = np.ascontiguousarray(np.stack([tr[c] for c in ("pc", "ins", "a", "b", "res", "next", "wr")], axis=1), dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(_lib.u32p)

    def ok(lst):
        lst = np.ascontiguousarray(lst, dtype=np.uint32).reshape(-1, 4)
        return mem_lib.emul_rv32mem_list_ok(ptr(rows), C.c_size_t(rows.shape[0]), ptr(lst), C.c_size_t(lst.shape[0]))

    assert ok(mem) == 1 and len(mem) == 12
    assert ok(mem[::-1]) == 0 and ok(mem[[1, 0] + list(range(2, 12))]) == 1      # the words of one ecall share a cycle ...
    swapped = mem.copy()
    swapped[[3, 4]] = swapped[[4, 3]]                                            # ... two loads do not
    assert swapped[3, 0] != swapped[4, 0] and ok(swapped) == 0
    assert ok(np.concatenate([mem[:4], mem[3:]])) == 0                           # a load's entry twice
    assert ok(mem[:-1]) == 0 and ok(mem[1:]) == 1 and ok(mem[4:]) == 0           # a load dropped; an ecall word may go
    alu = int(np.nonzero((tr["ins"] & 0x7F) == 0x13)[0][0])
    extra = np.concatenate([mem, [[alu, 5, 0, 0]]])
    assert ok(extra[np.argsort(extra[:, 0], kind="stable")]) == 0                # an entry at an ADDI row
    far = mem.copy()
    far[0, 1] = 1 << 30
    assert ok(far) == 0
    late = mem.copy()
    late[-1, 0] = rows.shape[0]
    assert ok(late) == 0                                                         # a cycle past the trace
    assert ok(np.zeros((0, 4))) == 0 and mem_lib.emul_rv32mem_list_ok(ptr(rows[:3]), C.c_size_t(3), ptr(rows), C.c_size_t(0)) == 1


def test_more_accesses_than_two_tables_hold_is_refused():
    """an ecall READ of 2^14 + 1 words in a 2^13-cycle shard: memop would be taller than twice the cpu table.
    rk_exec_rv32mem_sizes answers RK_ERR_CAPACITY and the numpy witness raises"""
    words = (1 << 14) + 1
    elf = GP.big_read_program(words)
    inp = list(range(1, words + 1))
    ex = X.execute(elf, inp, segment_limit_po2=13, record_trace=True)
    assert len(ex.segments) == 1 and ex.segments[0].po2 == 13 and len(ex.mem[0]) == words
    image = rv32elf.program_image(elf)
    s, (_c, data), (start, end, ecalls), mem = next(_shards(ex))
    with pytest.raises(ValueError, match="more accesses than twice"):
        rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)
    lib = _lib.load()
    st = X.Stepper(elf, inp, 13)
    try:
        more = C.c_int(0)
        _lib.check(None, lib.rk_exec_next_segment(st._h, C.byref(more)))
        a, b = C.c_size_t(0), C.c_size_t(0)
        assert lib.rk_exec_rv32mem_sizes(st._h, 0, C.byref(a), C.byref(b)) == _lib.RK_ERR_CAPACITY
    finally:
        st.close()
    # one word fewer fits: 2^14 rows
    ex = X.execute(GP.big_read_program(words - 1), inp, segment_limit_po2=13, record_trace=True)
    assert rv32mem.log_rows(len(ex.mem[0])) == 14
