"""TEST INFRASTRUCTURE for the Keccak-f[1600] chip (rk_keccak_chip_air / rk_keccak_chip_trace, include/raiko_hip.h):
`chip_rows`, a numpy restatement of the table written from the column definitions (theta / rho / pi / chi / iota as
raiko_amd/keccak.py states them, vectorised over the permutation slots), and `eval_rows` / `eval_pairs`, a step-list
evaluator vectorised over rows -- Air.check_trace walks 6 x 10^4 steps per row in Python, too slow for mutation tests."""
import numpy as np

from raiko_amd import keccak, p3
from raiko_amd.keccak_chip import Layout as L, limbs_of, min_rows

P = p3.P
_P = np.uint64(P)
_ONE = np.uint64(1)


def _rol(v, n):
    return (v << np.uint64(n)) | (v >> np.uint64(64 - n)) if n else v


def _bits(v):
    """(..., ) uint64 -> (..., 64) uint64 of 0 / 1, bit z at index z"""
    return (v[..., None] >> np.arange(64, dtype=np.uint64)) & _ONE


def chip_rows(states, ids=None, mult=None, rows=None):
    """states (n, 25) uint64, ids / mult canonical (None: 0 .. n - 1 / ones) -> (rows, width) canonical uint64.
    Slots past n -- the one the table's end cuts off too -- are the zero state, ID = M = 0"""
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 25)
    n = s.shape[0]
    rows = min_rows(n) if rows is None else rows
    slots = -(-rows // 25)
    assert slots >= n
    a = np.zeros((slots, 25), dtype=np.uint64)
    a[:n] = s
    idc, mc = np.zeros(slots, dtype=np.uint64), np.zeros(slots, dtype=np.uint64)
    idc[:n] = np.arange(n) if ids is None else np.asarray(ids, dtype=np.uint64)
    mc[:n] = 1 if mult is None else np.asarray(mult, dtype=np.uint64)
    out = np.zeros((slots * 25, L.WIDTH), dtype=np.uint64)
    for r in range(25):
        row = out[r::25]
        row[:, L.STEP + r] = 1
        row[:, L.A: L.A + 100] = limbs_of(a)
        lane = lambda x, y: a[:, x + 5 * y]
        c = [lane(x, 0) ^ lane(x, 1) ^ lane(x, 2) ^ lane(x, 3) ^ lane(x, 4) for x in range(5)]
        cp = [c[x] ^ c[(x - 1) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        ap = [[lane(x, y) ^ c[x] ^ cp[x] for y in range(5)] for x in range(5)]           # ap[x][y]
        b = [[None] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rol(ap[x][y], keccak._ROT[x][y])
        app = [[b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        appp00 = app[0][0] ^ np.uint64(keccak._RC[r] if r < 24 else 0)
        for x in range(5):
            row[:, L.C + 64 * x: L.C + 64 * x + 64] = _bits(c[x])
            row[:, L.CP + 64 * x: L.CP + 64 * x + 64] = _bits(cp[x])
            for y in range(5):
                i = x + 5 * y
                row[:, L.AP + 64 * i: L.AP + 64 * i + 64] = _bits(ap[x][y])
        flat = np.stack([app[i % 5][i // 5] for i in range(25)], axis=1)
        row[:, L.APP: L.APP + 100] = limbs_of(flat)
        row[:, L.APP00_BITS: L.APP00_BITS + 64] = _bits(app[0][0])
        row[:, L.APPP00: L.APPP00 + 4] = limbs_of(np.stack([appp00] * 25, axis=1))[:, :4]
        row[:, L.ID], row[:, L.M] = idc, mc
        row[:, L.M_IN], row[:, L.M_OUT] = (mc if r == 0 else 0), (mc if r == 24 else 0)
        a = flat.copy()
        a[:, 0] = appp00
    return out[:rows].copy()


def lanes_at(table, row):
    """the state in the columns A of row `row` of a canonical table -> (25,) uint64"""
    limbs = np.asarray(table[row, L.A: L.A + 100], dtype=np.uint64).reshape(25, 4)
    return limbs[:, 0] | limbs[:, 1] << np.uint64(16) | limbs[:, 2] << np.uint64(32) | limbs[:, 3] << np.uint64(48)


def outputs_of(table, n):
    """the outputs of the first n permutations of a canonical table: the columns A of their rows 24 -> (n, 25) uint64"""
    return np.stack([lanes_at(table, 25 * p + 24) for p in range(n)])


def _plan(air):
    """the step list with, per step, the values that die after it"""
    plan = getattr(air, "_eval_plan", None)
    if plan is None:
        steps = air.steps.tolist()
        last, nv = {}, 0
        for s, (op, a, b) in enumerate(steps):
            if op in (p3.ADD, p3.SUB, p3.MUL):
                last[a] = last[b] = s
            elif op in (p3.NEG, p3.ASSERT_ZERO):
                last[a] = s
            nv += op != p3.ASSERT_ZERO
        dies = [[] for _ in steps]
        for v, s in last.items():
            dies[s].append(v)
        plan = air._eval_plan = (steps, dies, nv)
    return plan


def eval_pairs(air, loc, nxt, first, last):
    """the AIR's main-trace constraints on m (row, next row) pairs: loc / nxt (width, m) canonical uint64, first / last
    (m,) 0 / 1 -> bool (m, n_constraints): constraint k fails on pair j (the asserts over the permutation trace never do:
    they are checked by proving, as in Air.check_trace)"""
    steps, dies, nv = _plan(air)
    m = loc.shape[1]
    first, last = np.asarray(first, dtype=np.uint64), np.asarray(last, dtype=np.uint64)
    vals = [None] * nv
    fails = np.zeros((m, air.n_constraints), dtype=bool)
    at = k = 0
    for s, (op, a, b) in enumerate(steps):
        if op == p3.ASSERT_ZERO:
            if vals[a] is not None:
                fails[:, k] = vals[a] != 0
            k += 1
        else:
            if op == p3.CONST:
                v = np.uint64(a)
            elif op == p3.LOCAL:
                v = loc[a]
            elif op == p3.NEXT:
                v = nxt[a]
            elif op == p3.IS_FIRST_ROW:
                v = first
            elif op == p3.IS_LAST_ROW:
                v = last
            elif op == p3.IS_TRANSITION:
                v = _ONE - last
            elif op in (p3.ADD, p3.SUB, p3.MUL):
                x, y = vals[a], vals[b]
                v = None if x is None or y is None else (x + y) % _P if op == p3.ADD else (x + _P - y) % _P if op == p3.SUB else x * y % _P
            elif op == p3.NEG:
                v = None if vals[a] is None else (_P - vals[a]) % _P
            else:                       # PERM_LOCAL / PERM_NEXT / CHALLENGE / CUMSUM (PUBLIC, PREP_*: the chip has none)
                assert op in (p3.PERM_LOCAL, p3.PERM_NEXT, p3.CHALLENGE, p3.CUMSUM), op
                v = None
            vals[at] = v
            at += 1
        for d in dies[s]:
            vals[d] = None
    return fails


def eval_rows(air, trace, rows_subset=None):
    """Air.check_trace restricted to the rows `rows_subset` (None: all) of a canonical trace (rows wrap around) ->
    sorted list of (row, constraint)"""
    t = np.ascontiguousarray(trace, dtype=np.uint64)
    n = t.shape[0]
    rows = np.arange(n) if rows_subset is None else np.asarray(sorted(rows_subset))
    fails = eval_pairs(air, np.ascontiguousarray(t[rows].T), np.ascontiguousarray(t[(rows + 1) % n].T), rows == 0, rows == n - 1)
    return sorted((int(rows[j]), int(k)) for j, k in zip(*np.nonzero(fails)))
