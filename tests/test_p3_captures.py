"""Everything rk_p3_verify_hashes and the four rk_p3_fri_* captures hand back, bit for bit against committed digests
(tests/golden/p3_capture_digests.json, written by the commit it names): the host verifier can be restructured, what it
records cannot move.  Three statements under parameter sets all five calls accept: tables tied by lookups (a
permutation batch), two plain tables of two heights (none), and the full SP1 set (100 queries: the threaded path)."""
import json
import os

import numpy as np
import pytest

import oracle_lib as o
from p3_cases import P3_CASES, air_of, init_of, sha, tables_of
from raiko_amd import fri_chip, fri_open, fri_reduce, fri_transcript, hal, p3

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "p3_capture_digests.json")))


def _lookup():
    return 1, dict(queries=5, pow_bits=2), p3.lookup_demo_tables(5, 3, seed=2), p3.to_mont([6])


def _cubic_fib():
    tables = [p3.Table.from_canonical(air_of("cubic", 5), *p3.cubic_trace(5, 5, seed=3)),
              p3.Table.from_canonical(air_of("fib", None), *p3.fibonacci_trace(3))]
    return 1, dict(queries=6, pow_bits=5), tables, p3.to_mont([4, 5])


def _full():
    case = "sp1_fib_k10_full"
    return P3_CASES[case][0], dict(P3_CASES[case][1]), tables_of(case), init_of(case)


STATEMENTS = {"lookup_demo_5_3": _lookup, "cubic5_fib3": _cubic_fib, "sp1_fib_k10_full": _full}


def digests(name):
    """{array name: {"words", "sha256"}} of every array the five calls return for the statement's oracle proof"""
    preset, over, tables, init = STATEMENTS[name]()
    o.oracle_set_params(preset, **over)
    try:
        pf = o.oracle_p3_prove(tables, init)
    finally:
        o.oracle_set_params()
    blob = hal.make_params(preset, **over)
    out = {}

    def add(key, a):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        out[key] = {"words": int(a.size), "sha256": sha(a)}

    rc, states = p3.verify_hashes(tables, pf, init, params=blob)
    assert rc == 0
    add("hashes.states", states)
    calls = {"openings": (fri_chip.fri_openings, ("publics", "records")),
             "inputs": (fri_reduce.fri_inputs, ("layout", "publics", "records")),
             "input_paths": (fri_open.fri_input_paths, ("publics", "records")),
             "transcript": (fri_transcript.fri_transcript, ("ops", "observed", "sampled"))}
    for call, (fn, names) in calls.items():
        rc, shape, *arrays = fn(tables, pf, init, blob)
        assert rc == 0
        add(call + ".shape", shape[:4])
        for n, a in zip(names, arrays):
            add(call + "." + n, np.array(a, dtype=np.uint32).reshape(-1) if n == "layout" else a)
    return out


@pytest.mark.parametrize("name", sorted(STATEMENTS))
def test_captures_match_the_committed_digests(name):
    assert sorted(GOLD["statements"]) == sorted(STATEMENTS)
    assert digests(name) == GOLD["statements"][name]


def test_an_empty_proof_is_a_verdict_not_an_argument_error():
    """no words at all reach the verifier as a proof of no words: shape mismatch (2) from rk_p3_verify and from every
    capture, with nothing but the verdict"""
    preset, over, tables, init = STATEMENTS["cubic5_fib3"]()
    blob = hal.make_params(preset, **over)
    none = np.zeros(0, dtype=np.uint32)
    assert p3.verify(tables, none, init, params=blob) == 2
    for fn, n in ((fri_chip.fri_openings, 2), (fri_reduce.fri_inputs, 3), (fri_open.fri_input_paths, 2), (fri_transcript.fri_transcript, 3)):
        assert fn(tables, none, init, blob) == (2,) + (None,) * (1 + n)
        assert fn(tables, none, (), blob)[0] == 2                   # nor do missing init words make it one
