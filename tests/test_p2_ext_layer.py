"""The external layer of poseidon2_core.hpp in its column-sums-first form, and the permutation variants that know
which output cells are read and which input cells are zero, on the host build of the header: tests/emul/emul_p2_forms.cpp
built as shipped and with -DRK_P2_EXT_M4_FIRST (the earlier forms), all four instances.  Words are compared, not
residues: the two forms compute the same exact integer w = M_E y, so every REDC output is the same 32-bit pattern.
The device side is tests/test_gpu_p2_kept_cells.py."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as o
import p2_edges as E

P = E.P
SRC = os.path.join(o.EMUL_DIR, "emul_p2_forms.cpp")
CSRC = os.path.join(o.ROOT, "raiko_amd", "csrc")
FORMS = {"full": 0, "digest": 1, "capacity": 2, "digest_nz16": 3, "digest_nz1": 4, "first4": 5, "last_rate_block": 6}


def kept(form, w):
    """the cells a form promises"""
    rate = w - 8
    return {0: range(w), 1: range(8), 2: range(rate, w), 3: range(8), 4: range(8), 5: range(4),
            6: range((rate - 1) // 4 * 4, (rate - 1) // 4 * 4 + 4)}[form]


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("p2_forms")

    def build(item):
        name, flags = item
        out = str(d / ("libp2f_%s.so" % name))
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", *flags, "-I", CSRC, "-o", out, SRC],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        lib = C.CDLL(out)
        i, vp = C.c_int, C.c_void_p
        for f, args in ((lib.p2f_layer_signed, [i, i, i, vp, vp]), (lib.p2f_layer_signed_blocks, [i, i, i, i, i, vp, vp]),
                        (lib.p2f_layer_unsigned, [i, i, i, i, vp]), (lib.p2f_permute, [i, i, i, vp, vp, vp, vp]),
                        (lib.p2f_m4_first, [])):
            f.restype, f.argtypes = C.c_int, args
        return name, lib

    with ThreadPoolExecutor(2) as ex:
        got = dict(ex.map(build, [("new", []), ("old", ["-DRK_P2_EXT_M4_FIRST"])]))
    assert got["new"].p2f_m4_first() == 0 and got["old"].p2f_m4_first() == 1
    return got


def m_ext_exact(y, m4):
    """w = M_E y on Python integers (no reduction): circ(2 M4, M4, ..., M4)"""
    m4m = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]] if m4 == 0 else [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]
    w = len(y)
    blk = [[sum(m4m[i][j] * y[b + j] for j in range(4)) for i in range(4)] for b in range(0, w, 4)]
    tot = [sum(b[i] for b in blk) for i in range(4)]
    return [blk[i // 4][i % 4] + tot[i % 4] for i in range(w)]


def signed_inputs(w, rng):
    m = P - 1
    col = [m if (i & 1) == 0 else -m for i in range(w)]            # alternating per column
    col2 = [m if (i & 3) < 2 else -m for i in range(w)]
    blk = [m if (i // 4) % 2 == 0 else -m for i in range(w)]       # alternating per block
    rows = [[m] * w, [-m] * w, col, [-x for x in col], col2, blk, [-x for x in blk], [0] * w]
    rows += [[int(x) for x in rng.integers(-m, m + 1, w)] for _ in range(200)]
    # one cell at an extreme, the rest at the other
    rows += [[m if i == j else -m for i in range(w)] for j in range(w)]
    return np.array(rows, dtype=np.int64).astype(np.int32)


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_signed_layer_words_equal_the_earlier_form_and_the_exact_integers(libs, w, m4):
    """m_ext_redc_s: random cells, every cell at +-(p - 1), signs alternating per column and per block; against the
    earlier form word for word, against REDC of the exact integer M_E y, and |w| within the stated 112 p"""
    rng = np.random.default_rng(7 * w + m4)
    y = np.ascontiguousarray(signed_inputs(w, rng))
    n = y.shape[0]
    out = {}
    for name, lib in libs.items():
        r = np.zeros_like(y)
        assert lib.p2f_layer_signed(w, m4, n, o.ptr(y), o.ptr(r)) == 0
        out[name] = r
    assert np.array_equal(out["new"], out["old"])
    worst = 0
    for t in range(n):
        wx = m_ext_exact([int(v) for v in y[t]], m4)
        worst = max(worst, max(abs(v) for v in wx))
        assert [int(v) for v in out["new"][t]] == [E.redc64(v) for v in wx], t
    assert worst < 112 * P and worst == (16 if m4 == 0 else 7) * (w // 4 + 1) * (P - 1)
    # only some blocks: the kept cells are the same words, the others untouched
    nb = w // 4
    for b0, bn in ((0, 2), (nb - 2, 2), (0, 1), ((w - 9) // 4, 1)):
        r = np.full_like(y, 12345)
        assert libs["new"].p2f_layer_signed_blocks(w, m4, b0, bn, n, o.ptr(y), o.ptr(r)) == 0
        sel = np.zeros(w, dtype=bool)
        sel[4 * b0: 4 * (b0 + bn)] = True
        assert np.array_equal(r[:, sel], out["old"][:, sel]) and np.all(r[:, ~sel] == 12345), (b0, bn)


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_unsigned_layer_words_equal_the_earlier_form(libs, w, m4):
    """m_ext_redc on canonical cells: random, every cell at p - 1, every cell at 0, alternating 0 / p - 1 per column
    and per block; and the zero-aware forms (cells from 16 on, from 1 on) against the general one on zero tails"""
    rng = np.random.default_rng(11 * w + m4)
    m = P - 1
    rows = [[m] * w, [0] * w, [m if (i & 1) == 0 else 0 for i in range(w)], [0 if (i & 1) == 0 else m for i in range(w)],
            [m if (i // 4) % 2 == 0 else 0 for i in range(w)], [0 if (i // 4) % 2 == 0 else m for i in range(w)]]
    rows += [[int(x) for x in rng.integers(0, P, w)] for _ in range(200)]
    s = np.array(rows, dtype=np.uint32)
    n = s.shape[0]

    def run(lib, nz, inp):
        c = np.ascontiguousarray(inp.copy())
        assert lib.p2f_layer_unsigned(w, m4, nz, n, o.ptr(c)) == 0
        return c

    want = run(libs["old"], w, s)
    assert np.array_equal(run(libs["new"], w, s), want)
    assert int(want.max()) < P + 53
    for nz in (16, 1):
        z = s.copy()
        z[:, nz:] = 0
        ref = run(libs["old"], w, z)
        assert np.array_equal(run(libs["new"], w, z), ref)
        assert np.array_equal(run(libs["new"], nz, z), ref), nz
        assert np.array_equal(run(libs["old"], nz, z), ref), nz


def run_form(lib, w, m4, form, tabs, inp):
    """-> the kept cells (canonical integers) of the form on `inp`"""
    m = E.mont_tables(*tabs)
    c = o.to_mont(np.array([int(x) for x in inp], dtype=np.uint64))
    assert lib.p2f_permute(w, m4, form, o.ptr(m[0]), o.ptr(m[1]), o.ptr(m[2]), o.ptr(c)) == 0
    out = [int(x) for x in o.from_mont(c)]
    return [out[i] for i in kept(form, w)]


def zero_tail(inp, nz):
    return list(inp[:nz]) + [0] * (len(inp) - nz)


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_kept_cell_and_zero_aware_permutations_equal_the_full_one(libs, w, m4):
    """every variant the kernels use against the first 8 / last 8 / chosen cells of the full permutation, both builds,
    preset and random tables, random and extreme inputs; the full form of the new build against the reference"""
    rng = np.random.default_rng(13 * w + m4)
    fams = E.table_families(w, m4)
    inputs = [[P - 1] * w, [0] * w] + [[int(x) for x in rng.integers(0, P, w)] for _ in range(6)]
    for fam in ("preset", "random"):
        tabs = fams[fam]
        for inp in inputs:
            for name, form in FORMS.items():
                x = zero_tail(inp, 16) if form == 3 else zero_tail(inp, 1) if form == 4 else inp
                ref = E.permute(x, m4, *tabs)
                want = [ref[i] for i in kept(form, w)]
                for lib in libs.values():
                    assert run_form(lib, w, m4, form, tabs, x) == want, (fam, name)


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_variants_at_the_aimed_worst_cases(emu, libs, w, m4):
    """the aimed cases of tests/p2_edges.py (entry states at the edges of the partial rounds' accumulators, worst
    tables) through every variant: the forms that assume zero cells get inputs with those cells zero, re-aimed"""
    bad = []
    for form in FORMS.values():
        base = E.base_tables(w)[1]
        inp = zero_tail(base, 16) if form == 3 else zero_tail(base, 1) if form == 4 else base
        for label, tabs, x, _ in E.aimed_cases(emu, w, m4, inp=inp):
            ref = E.permute(x, m4, *tabs)
            if run_form(libs["new"], w, m4, form, tabs, x) != [ref[i] for i in kept(form, w)]:
                bad.append((form, label))
    assert bad == []
