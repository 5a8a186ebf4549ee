"""The three public seal-bound routes (rk_seal_bound_words, rk_seal_bound_words_for, rk_seal_bound_words_params) pinned
over a grid of segment sizes, tap sets, protocol shapes and query counts: tests/golden/seal_bound_words.json holds the
values recorded from the library before the seal's shape (taps per register, Merkle cap, FRI round walk) moved into
shared helpers of taps.hpp.  `python tests/test_seal_bound_pin.py` rewrites the file from the library that is built."""
import ctypes as C
import json
import os

from raiko_amd import _lib, hal
from raiko_amd.segment import make_tapset, synthetic_tapset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seal_bound_words.json")

PO2 = [1, 2, 5, 8, 9, 13, 20, 22]
QUERIES = [1, 3, 50, 256]           # 256 = RK_MAX_QUERIES
# (name, tap set, n_globals): synthetic_segment's tap set at two widths, and the one of test_deep_tapset
TAPS = [
    ("synthetic-1-1-1", synthetic_tapset(1, 1, 1), 32),
    ("synthetic-16-16-224", synthetic_tapset(16, 16, 224), 32),
    ("deep", make_tapset([[(0, 1), (0, 1, 4)], [(0,), (0, 2)], [(0,), (0, 1), (0, 1, 2, 3), (0, 3), (1, 2), (0,), (0, 5)]]), 5),
]
# (name, preset, overrides): risc0, sp1, and the SHAPES of tests/test_params.py
SHAPES = [
    ("risc0", 0, {}),
    ("sp1", 1, {}),
    ("shape0", 0, dict(blowup_log2=1, fri_fold_log2=1, fri_min_degree=1, pow_bits=12)),
    ("shape1", 0, dict(blowup_log2=3, fri_fold_log2=2, fri_min_degree=16)),
    ("shape2", 0, dict(blowup_log2=1, fri_fold_log2=3, fri_min_degree=4, pow_bits=8)),
    ("shape3", 0, dict(blowup_log2=4, fri_fold_log2=4, fri_min_degree=64)),
    ("shape4", 0, dict(blowup_log2=2, fri_fold_log2=1, fri_min_degree=256, pow_bits=5)),
]


def grid_values():
    """{route: values in the order of the nested loops below}"""
    lib = _lib.load()
    plain, by_queries, by_params = [], [], []
    for _, taps, n_globals in TAPS:
        keep = []
        c = _lib.RkSegment()
        hal.fill_c_taps(c.taps, taps, keep)
        c.n_globals = n_globals
        for po2 in PO2:
            c.po2 = po2
            plain.append(int(lib.rk_seal_bound_words(C.byref(c))))
            for q in QUERIES:
                by_queries.append(int(lib.rk_seal_bound_words_for(C.byref(c), q)))
            for _, preset, over in SHAPES:
                for q in QUERIES:
                    blob = hal.make_params(preset, queries=q, **over)
                    by_params.append(int(lib.rk_seal_bound_words_params(C.byref(c), C.byref(blob))))
    return {"rk_seal_bound_words": plain, "rk_seal_bound_words_for": by_queries, "rk_seal_bound_words_params": by_params}


def axes():
    return {"taps": [t[0] for t in TAPS], "po2": PO2, "shapes": [s[0] for s in SHAPES], "queries": QUERIES}


def test_seal_bounds_equal_the_recorded_ones():
    with open(GOLDEN) as f:
        want = json.load(f)
    assert want["axes"] == axes()
    got = grid_values()
    assert len(got["rk_seal_bound_words_params"]) == len(TAPS) * len(PO2) * len(SHAPES) * len(QUERIES)
    for route, values in got.items():
        assert values == want[route], route
    assert any(v > 0 for v in got["rk_seal_bound_words_params"]) and 0 in got["rk_seal_bound_words_params"]   # po2 22 under blow-up 16


if __name__ == "__main__":
    out = {"axes": axes()}
    out.update(grid_values())
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
