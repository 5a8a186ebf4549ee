"""Poseidon2 (poseidon2_core.hpp) at the worst-case values of its unreduced arithmetic, on the host build of the same
headers, for all four shipped instances: an independent plain-integer reference, entry states aimed in the
representation the partial rounds' accumulators see, the bounds the header states checked on Python integers, the
two other selectable forms of the partial rounds, and a build that traps on signed overflow.  The device side of the
same cases is tests/test_gpu_p2_edges.py."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import oracle_lib as o
import p2_edges as E

P, H = E.P, E.H
TESTS = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_reference_matches_the_oracle(orc, w, m4):
    """E.permute against or_poseidon2_mix under the instance's preset tables and under random tables"""
    rng = np.random.default_rng(w + 10 * m4)
    rp = E.rounds_partial(w)
    fams = [E.preset_tables(w, m4), ([int(x) for x in rng.integers(0, P, 8 * w)], [int(x) for x in rng.integers(0, P, rp)],
                                     [int(x) for x in rng.integers(0, P, w)])]
    try:
        for ext, internal, diag in fams:
            m = E.mont_tables(ext, internal, diag)
            o.oracle_set_params(0 if w == 24 else 1, p2_width=w, p2_m4=m4, p2_rc_ext=m[0], p2_rc_int=m[1], p2_diag=m[2])
            for inp in [[P - 1] * w, [0] * w] + [[int(x) for x in rng.integers(0, P, w)] for _ in range(4)]:
                st = o.to_mont(np.array(inp, dtype=np.uint64))
                orc.or_poseidon2_mix(o.ptr(st))
                assert [int(x) for x in o.from_mont(st)] == E.permute(inp, m4, ext, internal, diag)
    finally:
        o.oracle_set_params()


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_aimed_entries_land_on_their_representatives(emu, w, m4):
    """the solved round-3 constants put the input where the partial rounds begin at the aimed raw cells: congruent,
    and at |x| >= h - 1 where +-h or +-(h - 1) was aimed (h and -h are the residues h and h + 1, whose representative
    is whichever of the two within p/2 + 53 m_ext_redc_s returns)"""
    for label, tabs, inp, raw in E.aimed_cases(emu, w, m4):
        assert E.entry_state(inp, m4, tabs[0]) == E.target_of_raw(raw)
        got = E.emul_entry_cells(emu, w, m4, tabs, inp)
        assert all((a - b) % P == 0 for a, b in zip(got, raw)), label
        assert all(abs(a) >= H - 1 for a, b in zip(got, raw) if abs(b) >= H - 1), label
        assert all(abs(a) <= P // 2 + 53 for a in got), label
        if label.endswith("/small"):                  # away from +-p/2 the representative is unique: 0, 1, -1 exactly
            assert got == raw, label


@pytest.mark.parametrize("w,m4", E.INSTANCES)
def test_host_permutation_at_the_edges(emu, w, m4):
    """emul_poseidon2_permute_cfg (the kernels' Core::permute) on every aimed case against the reference"""
    for label, tabs, inp, _ in E.aimed_cases(emu, w, m4):
        assert E.emul_permute(emu, w, m4, tabs, inp) == E.permute(inp, m4, *tabs), label


@pytest.mark.parametrize("w", [24, 16])
def test_partial_round_accumulators_stay_within_the_stated_bounds(emu, w):
    """partial_rounds() re-run on Python integers (E.partial_model) for every aimed case of both instances of the width:
    the exit equals the reference's state after the partial rounds (so the model is the kernel's arithmetic), and every
    accumulator stays within the bound the header states for it -- blocks of three rounds at both widths, and the
    one-round remainder block width 16 ends with.  The message gives the closest approach to every bound."""
    worst = {n: 0.0 for n in E.BOUNDS}
    for m4 in (0, 1):
        for label, tabs, inp, raw in E.aimed_cases(emu, w, m4):
            ext, internal, diag = tabs
            stream, k = E.emul_derived(emu, w, m4, tabs)
            cells = E.emul_entry_cells(emu, w, m4, tabs, inp)
            out, peak = E.partial_model(cells, stream, k, [x * E.R1 % P for x in internal], w)
            s = E.entry_state(inp, m4, ext)
            for rc in internal:
                s = E.partial_round(s, rc, diag)
            assert out == [x * E.R1 % P for x in s], label
            for n in E.BOUNDS:
                worst[n] = max(worst[n], peak[n] / E.BOUNDS[n][0])
    report = ", ".join("%s %.4f of %s" % (n, worst[n], E.BOUNDS[n][1]) for n in E.BOUNDS)
    print("W = %d: largest value / stated bound: %s" % (w, report))
    assert all(v <= 1.0 for v in worst.values()), report
    # the cases reach the edges they were built for
    assert worst["entry"] > 0.999 and worst["X"] > 0.5 and worst["T"] > 0.25 and worst["t"] > 0.25, report


@pytest.mark.parametrize("w", [24, 16])
def test_the_committed_worst_tables_are_still_the_best(emu, w):
    """E.WORST is what the seeded searches find: its diagonal scores as well as a fresh search's on the derived words
    (count at |c| >= 0.99 h, then |d_0|), and its internal constants drive the accumulators as hard as the best of a
    fresh search from the same entries"""
    ext, inp = E.base_tables(w)
    rp = E.rounds_partial(w)
    found = E.search_diag(w, seed=w)
    committed = E.table_score(emu, w, 0, (ext, [0] * rp, E.WORST[w]["diag"]))
    assert committed >= E.table_score(emu, w, 0, (ext, [0] * rp, found))
    # the search's numpy restatement of the stream words and the emulator's derive() count the same edge words
    stream, k = E.emul_derived(emu, w, 0, (ext, [0] * rp, E.WORST[w]["diag"]))
    predicted = sum(int(E.edge_count(E.diag_words(np.array([d], dtype=np.uint64), w))[0]) for d in E.WORST[w]["diag"][1:])
    assert predicted == sum(abs(c) >= int(0.99 * H) for c in stream) > len(stream) // 2
    entries = [E.emul_entry_cells(emu, w, 0, (E.aim(inp, 0, ext, E.target_of_raw(raw)), [0] * rp, E.WORST[w]["diag"]), inp)
               for raw in E.entry_patterns(w, stream).values()]
    best_rc, best = E.search_rc_int(w, stream, k, entries, seed=w, tries=400)
    rcm = [x * E.R1 % P for x in E.WORST[w]["rc_int"]]
    got = max(max(1 / m for n, m in E.margins(E.partial_model(e, stream, k, rcm, w)[1]).items() if n != "entry")
              for e in entries)
    assert got >= best - 1e-12, (got, best, best_rc)


# ---- the other selectable forms and the overflow-trapping build, compiled into tmp_path ----
VARIANTS = {"block2": ["-DRK_P2_BLOCK=2"], "direct": ["-DRK_P2_DIRECT"],
            "ubsan": ["-fsanitize=signed-integer-overflow", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module")
def variant_libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("emul_variants")

    def build(name):
        out = str(d / ("libemul_%s.so" % name))
        r = subprocess.run(o.emul_build_cmd(out, VARIANTS[name]), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        return name, out

    with ThreadPoolExecutor(len(VARIANTS)) as ex:
        return dict(ex.map(build, VARIANTS))


@pytest.mark.parametrize("name", ["block2", "direct"])
def test_other_partial_round_forms_at_the_edges(emu, variant_libs, name):
    """RK_P2_BLOCK=2 and RK_P2_DIRECT (kept selectable for A/B) on every aimed case of every instance"""
    lib = o.bind_emul(variant_libs[name])
    assert E.run_host_cases(lib, ref_emu=emu) == []


def test_no_signed_overflow_at_the_edges(variant_libs):
    """the shipped form built with -fsanitize=signed-integer-overflow, every aimed case of every instance, in a child
    process so that a trap fails this test instead of ending pytest"""
    code = ("import sys; sys.path.insert(0, %r); import oracle_lib as o, p2_edges as E; "
            "bad = E.run_host_cases(o.bind_emul(sys.argv[1])); print(bad); sys.exit(1 if bad else 0)") % TESTS
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code, variant_libs["ubsan"]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
