"""Constraint lists (rk_program) at saturating words: the generated kernel (rk_program_compile, circuit_jit.hip) keeps mix
states as unreduced 64-bit sums of products and places its folds by bounds tracked at generation time for worst-case
words (p - 1)^2.  Random LDE data sits far from that case; here every LDE word, global and mix word is p - 1, and
poly_mix is the Montgomery form of -1 or the word p - 1, on lists shaped to make the sums as long as the generator
allows: a long run of EQZ under one AND_COND, AND_CONDs nested inside each other, and the deep-nesting / spill shape
of test_gpu_program.py.  Interpreter and generated kernel against the oracle's literal interpretation, word for word."""
import numpy as np
import pytest

import oracle_lib as o
from raiko_amd import circuit_program as cp
from raiko_amd.segment import synthetic_tapset
from test_gpu_program import oracle_eval_check, run_eval_check

pytestmark = pytest.mark.gpu

P = o.P
N_GLOBALS, N_MIX = 4, 4


def _values(b):
    """every tap, global and mix word of the list as a field value (all p - 1 below), and their sum / difference"""
    vals = [b.get_tap(t) for t in range(12)] + [b.get_global(0, i) for i in range(N_GLOBALS)]
    vals += [b.get_global(1, i) for i in range(N_MIX)]
    vals += [b.sub(b.const(0), vals[0]), b.add(vals[1], vals[2])]       # 1 and p - 2
    return vals


def eqz_run(b, vals, n, start=0):
    x = b.true()
    for i in range(n):
        x = b.and_eqz(x, vals[(start + i) % len(vals)])
    return x


def long_run(b, vals):
    """120 EQZ inside one AND_COND, with runs before and after it in the outer state"""
    outer = eqz_run(b, vals, 40)
    x = b.and_cond(outer, vals[3], eqz_run(b, vals, 120, 5))
    for i in range(40):
        x = b.and_eqz(x, vals[(7 * i) % len(vals)])
    return x


def nested(b, vals, depth=6):
    """AND_CONDs inside AND_CONDs, each level with a run of 25 EQZ before and after its inner block"""
    def level(d):
        x = eqz_run(b, vals, 25, d)
        if d < depth:
            x = b.and_cond(x, vals[(d + 2) % len(vals)], level(d + 1))
        for i in range(25):
            x = b.and_eqz(x, vals[(d + i) % len(vals)])
        return x
    return level(0)


def stacked(b, vals, depth=10):
    """the spill shape of test_deeply_nested_blocks_spill_mix_states: outer states alive while inner ones are built"""
    if depth == 0:
        return eqz_run(b, vals, 30)
    outer = eqz_run(b, vals, 12, depth)
    return b.and_cond(outer, vals[(depth + 1) % len(vals)], stacked(b, vals, depth - 1))


@pytest.mark.parametrize("shape", ["long_run", "nested", "stacked"])
def test_saturated_lists_match_the_oracle(hal, shape):
    taps = synthetic_tapset(4, 3, 8)
    b = cp.ProgramBuilder(taps)
    vals = _values(b)
    ret = {"long_run": long_run, "nested": nested, "stacked": stacked}[shape](b, vals)
    steps = b.array()
    interp, jit = cp.Program(steps, ret, taps), cp.Program(steps, ret, taps)
    jit.compile(hal)
    po2 = 6
    d = 4 << po2
    lde = [np.full((int(w), d), P - 1, dtype=np.uint32) for w in taps.group_size]
    glob = np.full(N_GLOBALS, P - 1, dtype=np.uint32)
    mix = np.full(N_MIX, P - 1, dtype=np.uint32)
    minus_one = int(o.to_mont([P - 1])[0])
    for pm in (np.array([minus_one, 0, 0, 0], dtype=np.uint32), np.full(4, P - 1, dtype=np.uint32)):
        want = oracle_eval_check(interp, taps, po2, lde, glob, mix, pm)
        assert np.array_equal(run_eval_check(hal, interp, po2, lde, glob, mix, pm), want), (shape, pm)
        assert np.array_equal(run_eval_check(hal, jit, po2, lde, glob, mix, pm), want), (shape, pm)
