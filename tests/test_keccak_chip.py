"""The Keccak-f[1600] chip (rk_keccak_chip_air / rk_keccak_chip_trace, include/raiko_hip.h; raiko_amd/keccak_chip.py) on
the CPU: the numpy restatement of its table (tests/keccak_chip_ref.py) computes Keccak-f[1600]; the library-written AIR
accepts it and pins every committed cell; the oracle proves a claims table against the chip, both verifiers agree on
every verdict and forged statements are refused; the lane body of the rows kernel, run under g++ (and once more as a
program of its own under AddressSanitizer and UBSan), writes that table word for word.  The chip's shape is
p3-keccak-air's, RECALLED (the crate is outside the reference tree); everything here is bit-exact."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import keccak_chip_ref as R
import oracle_lib as o
from raiko_amd import hal, keccak, keccak_chip as K, p3

P = o.P
L = K.Layout
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PERM_ASSERTS = 20         # the lookup argument's own: two batches x 4, first / transition / last 3 x 4


def f1600(lanes):
    a = [[int(lanes[x + 5 * y]) for y in range(5)] for x in range(5)]
    return K.lanes_of(keccak._f1600(a))


def one_round(lanes, rc):
    """one round of raiko_amd.keccak._f1600, on 25 lanes"""
    a = [[int(lanes[x + 5 * y]) for y in range(5)] for x in range(5)]
    c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
    d = [c[(x - 1) % 5] ^ keccak._rol(c[(x + 1) % 5], 1) for x in range(5)]
    a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
    b = [[0] * 5 for _ in range(5)]
    for x in range(5):
        for y in range(5):
            b[y][(2 * x + 3 * y) % 5] = keccak._rol(a[x][y], keccak._ROT[x][y])
    a = [[b[x][y] ^ ((~b[(x + 1) % 5][y]) & b[(x + 2) % 5][y]) & keccak._M for y in range(5)] for x in range(5)]
    a[0][0] ^= rc
    return K.lanes_of(a)


def edge_states():
    """zero, all-ones, each lane = 1 alone, lane (0, 0) = 2^63, lane (4, 4) = 2^63, eight random states"""
    s = np.zeros((37, 25), dtype=np.uint64)
    s[1] = np.uint64(keccak._M)
    for i in range(25):
        s[2 + i, i] = 1
    s[27, 0] = s[28, 24] = np.uint64(1 << 63)
    s[29:] = np.random.default_rng(1600).integers(0, 1 << 64, size=(8, 25), dtype=np.uint64)
    return s


@pytest.fixture(scope="module")
def air():
    return K.keccak_chip_air()


@pytest.fixture(scope="module")
def five():
    """the n = 5 table (128 rows: three rows of a sixth permutation), with ids and multiplicities of its own"""
    states = np.random.default_rng(5).integers(0, 1 << 64, size=(5, 25), dtype=np.uint64)
    rows = R.chip_rows(states, ids=[7, 8, 9, 10, 11], mult=[1, 3, 0, 2, 1])
    rows.setflags(write=False)
    return states, rows


# ------------------------------------------------------------------------------------------------ 1. reference outputs
def test_the_restatement_computes_keccak_f1600():
    states = edge_states()
    rows = R.chip_rows(states)
    assert rows.shape == (1024, L.WIDTH) == (K.min_rows(37), 2537) and int(rows.max()) < 1 << 16
    outs = R.outputs_of(rows, len(states))
    for i, s in enumerate(states):
        assert np.array_equal(outs[i], f1600(s)), i
    # rows 1 .. 23 of A are the successive round states (row 24: the output)
    for p in (1, 30):
        cur = states[p]
        for r in range(24):
            cur = one_round(cur, keccak._RC[r])
            assert np.array_equal(R.lanes_at(rows, 25 * p + r + 1), cur), (p, r)


def test_the_restatement_against_hashlib_sha3_256():
    msgs = [b"", b"abc", bytes(range(135))]
    blocks = []
    for m in msgs:                                          # SHA3-256: rate 136, padding 0x06 .. 0x80, one block
        blk = bytearray(m) + b"\x06" + bytes(135 - len(m))
        blk[135] |= 0x80
        blocks.append(np.frombuffer(bytes(blk) + bytes(64), dtype="<u8"))
    outs = R.outputs_of(R.chip_rows(np.array(blocks)), 3)
    for m, out in zip(msgs, outs):
        assert out.astype("<u8").tobytes()[:32] == hashlib.sha3_256(m).digest()


# ------------------------------------------------------------------------------------------------ 2. the AIR
def test_air_shape(air):
    info = air.info()
    assert info["max_degree"] == 3 and info["log_quotient_degree"] == 1 == air.log_quotient_degree()
    assert air.width == L.WIDTH == 2537 == int(o_lib().rk_keccak_chip_width()) and air.perm_width == 12
    assert info["n_constraints"] == air.n_constraints == 2988 + N_PERM_ASSERTS
    its = air.interactions
    assert [it.bus for it in its] == [15, 16, 17, 18] and all(it.kind == p3.RECEIVE and not it.mult_is_const for it in its)
    assert [it.mult for it in its] == [L.M_IN, L.M_IN, L.M_OUT, L.M_OUT]
    assert max(len(it.value_cols) for it in its) == 51
    assert len({c for it in its for c in it.value_cols + [it.mult]}) == 103
    assert its[0].value_cols == its[2].value_cols == [L.ID] + list(range(L.A, L.A + 50))
    assert its[1].value_cols == its[3].value_cols == [L.ID] + list(range(L.A + 50, L.A + 100))
    other = K.keccak_chip_air(hal.make_params(0), bus=30)       # risc0's extension: the same main constraints
    n_main = int(np.flatnonzero(air.steps[:, 0] == p3.ASSERT_ZERO)[2987]) + 1
    assert np.array_equal(other.steps[:n_main], air.steps[:n_main]) and not np.array_equal(other.steps, air.steps)
    assert [it.bus for it in other.interactions] == [30, 31, 32, 33]


def o_lib():
    from raiko_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("n,rows", [(1, 32), (2, 64), (5, 128), (1, 64)])
def test_air_accepts_the_restatement(air, n, rows):
    states = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 25), dtype=np.uint64)
    table = R.chip_rows(states, rows=rows)
    assert table.shape == (rows, L.WIDTH) and (rows == K.min_rows(n) or (n, rows) == (1, 64))
    assert R.eval_rows(air, table) == []
    assert int(table[:, L.M].sum()) == 25 * n and int(table[25 * n:, L.ID].sum()) == 0      # the padding slots: M = ID = 0


def test_the_vectorised_evaluator_is_check_trace(air):
    table = R.chip_rows(np.random.default_rng(32).integers(0, 1 << 64, size=(1, 25), dtype=np.uint64))
    assert table.shape[0] == 32 and air.check_trace(table) == [] == R.eval_rows(air, table)
    broken = table.copy()
    for r, c in ((3, L.AP + 700), (10, L.A + 17), (24, L.STEP + 24), (31, L.M), (0, L.C + 5)):
        broken[r, c] = (int(broken[r, c]) + 1) % P
    want = sorted(air.check_trace(broken))
    assert want == R.eval_rows(air, broken) and len({r for r, _ in want}) >= 6
    assert R.eval_rows(air, broken, [9, 10]) == [v for v in want if v[0] in (9, 10)]


# ------------------------------------------------------------------------------------------------ 3. every cell is pinned
def test_every_committed_cell_is_pinned(air, five):
    """One cell changed by +1: some main-trace constraint fails at the row before or at the row itself.  Constraints read a
    row and its successor only, so those two rows are all that is evaluated, batched over the variants."""
    _states, rows = five
    n_rows = rows.shape[0]
    n_main = air.n_constraints - N_PERM_ASSERTS
    a_cols = list(range(L.A, L.A + 100))
    mid, first, last = 25 + 11, 25, 25 + 24                  # a middle row, row 0 and row 24 (the output row) of permutation 1
    # + 1 in every column of the middle row (ID and M too: only they reach the two constraints that carry them on), in the A
    # columns also in rows 0 and 24 of permutation 1, and in STEP[0] of the table's first row (only a change there reaches
    # the first-row constraint).  On top, - 1 in the bit columns of the middle row: + 1 leaves a 0 bit boolean, - 1 does
    # not, so between them every boolean constraint is reached
    bit_cols = list(range(L.STEP, L.STEP + 25)) + list(range(L.C, L.C + 320)) + list(range(L.AP, L.AP + 1600)) + \
        list(range(L.APP00_BITS, L.APP00_BITS + 64))
    variants = [(mid, c, 1) for c in range(L.WIDTH)] + [(first, c, 1) for c in a_cols] + [(last, c, 1) for c in a_cols] + [(0, L.STEP, 1)] + \
        [(mid, c, P - 1) for c in bit_cols]
    hit = set()
    for lo in range(0, len(variants), 700):
        chunk = variants[lo: lo + 700]
        m = len(chunk)
        loc, nxt = np.empty((L.WIDTH, 2 * m), dtype=np.uint64), np.empty((L.WIDTH, 2 * m), dtype=np.uint64)
        at = np.empty(2 * m, dtype=np.int64)
        for j, (r, c, delta) in enumerate(chunk):            # pair 2 j: row r - 1 with the changed row after it; pair 2 j + 1: the changed row
            changed = rows[r].copy()
            changed[c] = (int(changed[c]) + delta) % P
            loc[:, 2 * j], nxt[:, 2 * j], at[2 * j] = rows[(r - 1) % n_rows], changed, (r - 1) % n_rows
            loc[:, 2 * j + 1], nxt[:, 2 * j + 1], at[2 * j + 1] = changed, rows[r + 1], r
        fails = R.eval_pairs(air, loc, nxt, at == 0, at == n_rows - 1)
        assert not fails[:, n_main:].any()
        for j, (r, c, delta) in enumerate(chunk):
            before, here = np.flatnonzero(fails[2 * j]), np.flatnonzero(fails[2 * j + 1])
            if r == first and c in a_cols:
                # A in row 0 is the free input: nothing ties it to the row before; the rest of its own row no longer fits
                assert before.size == 0 and here.size > 0, (r, c, delta)
            else:
                assert before.size + here.size > 0, (r, c, delta)
            hit |= set(before.tolist()) | set(here.tolist())
    assert sorted(set(range(n_main)) - hit) == []


# ------------------------------------------------------------------------------------------------ 4. proofs
def test_proof_level_refusals():
    over = dict(queries=4, pow_bits=2)
    o.oracle_set_params(1, **over)
    try:
        blob = hal.make_params(1, **over)
        chip_air, claims_air = K.keccak_chip_air(blob), K.claims_air()
        assert claims_air.width == 55 and claims_air.check_trace(K.claims_rows(np.zeros((1, 25)), np.ones((1, 25)))) == []
        states = np.random.default_rng(2).integers(0, 1 << 64, size=(2, 25), dtype=np.uint64)
        chip = R.chip_rows(states)
        outs = R.outputs_of(chip, 2)
        claims = K.claims_rows(states, outs)
        assert chip.shape[0] == 64 and claims.shape == (8, 55)

        def verdict(claims_rows, chip_rows):
            tabs = [p3.Table.from_canonical(claims_air, claims_rows), p3.Table.from_canonical(chip_air, chip_rows)]
            pf = o.oracle_p3_prove(tabs)
            a, b = o.oracle_p3_verify(tabs, pf), p3.verify(tabs, pf, params=blob)
            assert a == b
            return a

        assert verdict(claims, chip) == 0
        off = claims.copy()                                   # a claimed output limb that the permutation does not give
        off[6, 1 + 9] = (int(off[6, 1 + 9]) + 1) % (1 << 16)
        assert verdict(off, chip) == 8
        swapped = claims.copy()                               # the two permutations' IDs swapped in the claims only
        swapped[:8, 0] = 1 - swapped[:8, 0]
        assert verdict(swapped, chip) == 8
        cut = chip.copy()                                     # M = 1 on the permutation the table's end cuts off: its input
        cut[50:, L.M] = 1                                     # is received, its output never
        cut[50, L.M_IN] = 1
        assert R.eval_rows(chip_air, cut) == [] and verdict(claims, cut) == 8
        forged = chip.copy()                                  # a prover-side forgery: one limb of A'' is not the round's
        forged[30, L.APP + 41] = (int(forged[30, L.APP + 41]) + 1) % (1 << 16)
        assert verdict(claims, forged) == 3
        # M changes in the middle of a permutation: the chip takes the input of permutation 0 and gives the output of
        # permutation 1, and the claims ask for just that, so the cumulative sums cancel -- the constraint that carries
        # M on is all that stands against pairing one permutation's input with another's output
        drift, mixed = chip.copy(), claims.copy()
        drift[12:25, L.M] = drift[24, L.M_OUT] = 0
        drift[25:37, L.M] = drift[25, L.M_IN] = 0
        mixed[2:6, 51:] = 0
        assert claims_air.check_trace(mixed) == [] and {r for r, _ in R.eval_rows(chip_air, drift)} == {11, 36}
        assert verdict(mixed, drift) == 3
    finally:
        o.oracle_set_params()


# ------------------------------------------------------------------------------------------------ 5. the lane body under g++
@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_keccak_chip") / "libemul_keccak_chip.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", "emul_keccak_chip.cpp")], check=True, capture_output=True)
    lib = C.CDLL(so)
    lib.emul_keccak_chip_width.restype = C.c_uint32
    lib.emul_keccak_chip_rows.restype = None
    lib.emul_keccak_chip_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    return lib


def lane_body_rows(lib, states, ids=None, mult=None, rows=None):
    s = np.ascontiguousarray(states, dtype=np.uint64)
    n = s.shape[0]
    rows = K.min_rows(n) if rows is None else rows
    trace = np.full((rows, L.WIDTH), 0xFFFFFFFF, dtype=np.uint32)
    out = np.zeros((n, 25), dtype=np.uint64)
    im, mm = (None if v is None else p3.to_mont(v) for v in (ids, mult))
    lib.emul_keccak_chip_rows(s.ctypes.data, None if im is None else im.ctypes.data, None if mm is None else mm.ctypes.data, n, rows,
                              trace.ctypes.data, out.ctypes.data)
    return trace, out


@pytest.mark.parametrize("n,rows", [(1, 32), (2, 64), (5, 128), (1, 64)])
def test_lane_body_writes_the_restatement(emul_lib, n, rows):
    assert emul_lib.emul_keccak_chip_width() == L.WIDTH
    rng = np.random.default_rng(10 + n)
    states = rng.integers(0, 1 << 64, size=(n, 25), dtype=np.uint64)
    got, out = lane_body_rows(emul_lib, states, rows=rows)
    assert np.array_equal(got, p3.to_mont(R.chip_rows(states, rows=rows)))
    assert all(np.array_equal(out[i], f1600(states[i])) for i in range(n))
    ids, mult = rng.integers(0, P, size=n), rng.integers(0, 4, size=n)
    got, out2 = lane_body_rows(emul_lib, states, ids, mult, rows)
    assert np.array_equal(got, p3.to_mont(R.chip_rows(states, ids, mult, rows))) and np.array_equal(out, out2)


def test_lane_body_on_the_edge_states(emul_lib):
    states = edge_states()
    got, out = lane_body_rows(emul_lib, states)
    assert np.array_equal(got, p3.to_mont(R.chip_rows(states)))
    assert all(np.array_equal(out[i], f1600(s)) for i, s in enumerate(states))


def test_lane_body_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = str(tmp_path / "keccak_chip_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "asan", "keccak_chip_main.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "keccak_chip_main ok" in r.stdout


def test_entry_points_refuse_malformed_arguments():
    lib = o_lib()
    h = C.c_void_p()
    assert lib.rk_keccak_chip_air(None, 15, None) == -1
    assert lib.rk_keccak_chip_air(None, P - 3, C.byref(h)) == -1            # bus + 3 not canonical
    bad = hal.make_params(1)
    bad.p2_width = 20
    assert lib.rk_keccak_chip_air(C.byref(bad), 15, C.byref(h)) == -1
    assert lib.rk_keccak_chip_trace(None, None, None, None, 1, 32, None, None) == -1
