"""The partial rounds of the width-24 permutation in blocks of rounds (poseidon2_core.hpp:partial_rounds) at the
edges of their value ranges: host code, the same Core::permute the kernels run.  The accumulators there are signed
64-bit sums of products by centred constants, so what can overflow is reached by constants near 0, 1, -1 and +-p/2
and by cells that are extreme field values when the partial rounds begin (chosen there, then carried back through
the first half of the permutation)."""
import numpy as np
import pytest

import oracle_lib as o
from test_emul_kernels import _py_permute

P = o.P
H = (P - 1) // 2
M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]
INV7 = pow(7, -1, P - 1)


def _m_ext_matrix():
    return [[(2 if i // 4 == j // 4 else 1) * M4[i % 4][j % 4] for j in range(24)] for i in range(24)]


def _inverse_mod_p(m):
    n = len(m)
    a = [row[:] + [int(i == j) for j in range(n)] for i, row in enumerate(m)]
    for c in range(n):
        r = next(r for r in range(c, n) if a[r][c] % P)
        a[c], a[r] = a[r], a[c]
        iv = pow(a[c][c], -1, P)
        a[c] = [x * iv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


MINV = _inverse_mod_p(_m_ext_matrix())


def _apply(m, v):
    return [sum(a * b for a, b in zip(row, v)) % P for row in m]


def _state_entering_partial_rounds(cells, ext):
    """the input whose first external layer and four full rounds give `cells`"""
    s = list(cells)
    for r in range(3, -1, -1):
        s = _apply(MINV, s)
        s = [(pow(x, INV7, P) - ext[r * 24 + i]) % P for i, x in enumerate(s)]
    return _apply(MINV, s)


EDGE = [0, 1, P - 1, H, H + 1, H - 1, H + 2, 2, P - 2]


def _diag(kind, rng):
    if kind == "edges":
        return [EDGE[i % len(EDGE)] for i in range(24)]
    if kind == "half":  # every multiplier as large as a centred constant gets, alternating signs
        return [H if i % 2 else H + 1 for i in range(24)]
    if kind == "minus_one":
        return [P - 1] * 24
    if kind == "zero_one":
        return [i % 2 for i in range(24)]
    return [int(x) for x in rng.integers(0, P, 24)]


@pytest.mark.parametrize("kind", ["edges", "half", "minus_one", "zero_one", "random"])
def test_partial_round_blocks_at_the_edges(emu, kind):
    rng = np.random.default_rng(2024)
    diag = _diag(kind, rng)
    ext = [int(x) for x in rng.integers(0, P, 192)]
    entries = [[P - 1] * 24, [H] * 24, [H + 1] * 24, [0] * 24, [1] * 24,
               [(H if i % 2 else H + 1) for i in range(24)],
               [EDGE[(i * 5) % len(EDGE)] for i in range(24)]]
    for internal in ([P - 1] * 21, [H] * 21, [int(x) for x in rng.integers(0, P, 21)]):
        m = [o.to_mont(np.array(x, dtype=np.uint64)) for x in (ext, internal, diag)]
        for cells in entries:
            c = _state_entering_partial_rounds(cells, ext)
            st = o.to_mont(np.array(c, dtype=np.uint64))
            emu.emul_poseidon2_permute_with(st.ctypes.data, m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data)
            assert [int(x) for x in o.from_mont(st)] == _py_permute(c, ext, internal, diag)


def test_partial_round_blocks_random_states_extreme_diagonal(emu):
    rng = np.random.default_rng(99)
    ext = [int(x) for x in rng.integers(0, P, 192)]
    internal = [int(x) for x in rng.integers(0, P, 21)]
    diag = [H + (i % 2) for i in range(24)]
    m = [o.to_mont(np.array(x, dtype=np.uint64)) for x in (ext, internal, diag)]
    for _ in range(200):
        c = [int(x) for x in rng.integers(0, P, 24)]
        st = o.to_mont(np.array(c, dtype=np.uint64))
        emu.emul_poseidon2_permute_with(st.ctypes.data, m[0].ctypes.data, m[1].ctypes.data, m[2].ctypes.data)
        assert [int(x) for x in o.from_mont(st)] == _py_permute(c, ext, internal, diag)
