"""The Keccak-256 sponge table (rk_keccak_sponge_air / rk_keccak_sponge_trace, include/raiko_hip.h;
raiko_amd/keccak_sponge.py) on the CPU: the numpy restatement of its table (tests/keccak_sponge_ref.py) computes
Keccak-256; the library-written AIR accepts it and pins every committed cell; the oracle proves [sponge, chip], the
verifier adds the receive claims of ITS messages and digests, and forged statements and forged witnesses are refused;
the lane body of the rows kernel, run under g++ (and once more as a program of its own under AddressSanitizer and
UBSan), writes that table word for word.  Everything here is bit-exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import keccak_chip_ref as CR
import keccak_sponge_ref as R
import oracle_lib as o
import p3_ref as PR
import p3_ref_claims as RC
from raiko_amd import _lib, hal, keccak, keccak_chip as K, keccak_sponge as S, p3

P = o.P
L = S.Layout
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAIN = 3077 - 28           # the lookup argument's own 28: four batches x 4, first / transition / last 3 x 4
FLAGS = list(range(L.MSG, L.WIDTH))


@pytest.fixture(scope="module")
def air():
    return S.keccak_sponge_air()


@pytest.fixture(scope="module")
def five():
    """the (1, 2, 1, 3, 1) set: 8 groups in 32 rows, two padding groups and two rows of an eleventh"""
    msgs = R.set_12131()
    rows = R.sponge_rows(msgs)
    rows.setflags(write=False)
    return msgs, rows


# ------------------------------------------------------------------------------------------------ 1. the restatement
def by_hand(message):
    """Keccak-256 absorbed block by block with raiko_amd.keccak._f1600 -> (inputs, outputs), 25 lanes each"""
    b = bytearray(message) + b"\x01"
    b += bytes(-len(b) % 136)
    b[-1] |= 0x80
    a = [[0] * 5 for _ in range(5)]
    ins, outs = [], []
    for off in range(0, len(b), 136):
        for i in range(17):
            a[i % 5][i // 5] ^= int.from_bytes(b[off + 8 * i: off + 8 * i + 8], "little")
        ins.append(K.lanes_of(a))
        a = keccak._f1600(a)
        outs.append(K.lanes_of(a))
    return np.array(ins), np.array(outs)


def test_the_restatement_computes_keccak256():
    sizes = [0, 1, 135, 136, 137, 271, 272, 273]
    rng = np.random.default_rng(1000)
    msgs = [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in sizes + [1000]]
    blocks, first = S.pad_blocks(msgs)
    assert np.diff(first.astype(int)).tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 8] and blocks.shape == (23, 17)
    rows = R.sponge_rows(msgs)
    assert rows.shape == (128, L.WIDTH) == (S.min_rows(23), 2458) and int(rows.max()) < max(1 << 16, 3 * 23)
    assert R.digests_of(rows) == [keccak.keccak256(m) for m in msgs]
    ins, outs = R.states_of(rows, 23)
    want = [by_hand(m) for m in msgs]
    assert np.array_equal(ins, np.concatenate([w[0] for w in want])) and np.array_equal(outs, np.concatenate([w[1] for w in want]))
    # the X rows hold the padded bytes; PID counts the groups; BLK / NBLK / FIRST / LAST follow the block counts
    assert rows[0:69:3, L.V: L.V + 68].astype("<u2").tobytes() == blocks.astype("<u8").tobytes()
    assert rows[:69, L.PID].tolist() == [b for b in range(23) for _ in range(3)] and not rows[69:].any()
    assert rows[2:69:3, L.S_DIG].tolist() == [int(b + 1 in first) for b in range(23)]
    assert rows[rows[:, L.S_DIG] == 1, L.NBLK].tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 8]


# ------------------------------------------------------------------------------------------------ 2. the AIR
def test_air_shape(air):
    lib = _lib.load()
    info = air.info()
    assert info["max_degree"] <= 3 and info["log_quotient_degree"] == 1 == air.log_quotient_degree()
    assert air.width == L.WIDTH == int(lib.rk_keccak_sponge_width()) and int(lib.rk_keccak_sponge_rows_per_block()) == S.ROWS_PER_BLOCK == 3
    assert info["n_constraints"] == air.n_constraints == N_MAIN + 28
    its = air.interactions
    assert len(its) == 7 and [it.bus for it in its] == list(range(15, 22)) and K.BUS_KECCAK == 15
    assert all(it.kind == p3.SEND and not it.mult_is_const for it in its)
    assert [it.mult for it in its] == [L.S_IN, L.S_IN, L.S_OUT, L.S_OUT, L.S_MSG, L.S_MSG, L.S_DIG]
    assert [len(it.value_cols) for it in its] == [51, 51, 51, 51, 36, 36, 18] and max(len(it.value_cols) for it in its) <= 64
    assert len({c for it in its for c in it.value_cols + [it.mult]}) == 108 <= 120
    chip = K.keccak_chip_air()                       # the chip's receives take what the first four send, tuple for tuple
    assert [(it.bus, len(it.value_cols)) for it in chip.interactions] == [(it.bus, len(it.value_cols)) for it in its[:4]]
    assert its[4].value_cols == [L.MSG, L.BLK] + list(range(34)) and its[5].value_cols == [L.MSG, L.BLK] + list(range(34, 68))
    assert its[6].value_cols == [L.MSG, L.NBLK] + list(range(16))
    other = S.keccak_sponge_air(hal.make_params(0), bus=30)       # risc0's extension: the same main constraints
    n_main = int(np.flatnonzero(air.steps[:, 0] == p3.ASSERT_ZERO)[N_MAIN - 1]) + 1
    assert np.array_equal(other.steps[:n_main], air.steps[:n_main]) and not np.array_equal(other.steps, air.steps)
    assert [it.bus for it in other.interactions] == list(range(30, 37))


def test_python_restates_the_layout_and_the_launch_constants():
    """keccak_sponge.Layout is kc::KeccakSpongeLayout, WAVES_PER_BLOCK / CHAIN_WAVES_PER_BLOCK are KS_WAVES / KS_CHAIN_WAVES:
    read from the sources, so that the shapes of the GPU test stay the kernels' thresholds"""
    hpp = open(os.path.join(ROOT, "raiko_amd", "csrc", "keccak_sponge.hpp")).read()
    hip = open(os.path.join(ROOT, "raiko_amd", "csrc", "keccak_sponge.hip")).read()
    assert int(re.search(r"constexpr unsigned KS_WAVES = (\d+);", hip).group(1)) == S.WAVES_PER_BLOCK
    assert int(re.search(r"constexpr unsigned KS_CHAIN_WAVES = (\d+);", hip).group(1)) == S.CHAIN_WAVES_PER_BLOCK
    named = dict(re.findall(r"\b([A-Z_]+) = (\d+)[,;]", hpp[hpp.index("struct KeccakSpongeLayout"): hpp.index("// ---- the rows")]))
    for name in ("MSG", "BLK", "NBLK", "PID", "KX", "KI", "KO", "REAL", "FIRST", "LAST", "S_IN", "S_OUT", "S_MSG", "S_DIG", "WIDTH"):
        assert int(named[name]) == getattr(L, name), name
    assert int(named["ROWS"]) == S.ROWS_PER_BLOCK and int(named["RATE_LANES"]) * 8 == S.RATE
    for fn, at in (("v", L.V), ("prev", L.PREV), ("mb", L.MB), ("pb", L.PB), ("xr", L.XR)):
        assert int(re.search(r"uint32_t %s\([^)]*\) \{ return (\d+)? ?\+? ?" % fn, hpp).group(1) or 0) == at, fn


@pytest.mark.parametrize("case", ["empty", "five", "twice"])
def test_air_accepts_the_restatement(air, five, case):
    table = {"empty": lambda: R.sponge_rows([b""]), "five": lambda: five[1], "twice": lambda: R.sponge_rows(five[0], rows=64)}[case]()
    assert table.shape[0] == {"empty": 4, "five": 32, "twice": 64}[case]
    assert air.check_trace(table) == [] == CR.eval_rows(air, table)
    n_real = int(table[:, L.REAL].sum())
    assert n_real % 3 == 0 and table[:n_real, L.REAL].all() and not table[n_real:].any()      # real groups, then zero rows


def test_every_committed_cell_is_pinned(air, five):
    """One cell changed by + 1 or - 1: some main-trace constraint fails at the row before or at the row itself; between
    them the variants reach every constraint.  Constraints read a row and its successor only, so those two pairs are all
    that is evaluated, batched over the variants."""
    _msgs, rows = five
    n_rows = rows.shape[0]
    # every column of the X, I and O row of a middle block (block 1 of the three-block message: rows 15, 16, 17) and of a
    # padding row (26); on top the flags and PREV where only a special row reaches a constraint: the table's first row
    # (0), an X row after a LAST O row (9), the X row after an O row that continues (18), the last real row (23), the
    # first padding row (24) and the table's last row (31)
    assert rows[15:18, L.KX: L.KX + 3].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1]] and not rows[15, [L.FIRST, L.LAST]].any()
    assert rows[8, L.S_DIG] == rows[23, L.S_DIG] == rows[9, L.FIRST] == 1 and rows[17, L.S_DIG] == 0 and not rows[24:].any()
    variants = [(r, c, d) for r in (15, 16, 17, 26) for c in range(L.WIDTH) for d in (1, P - 1)]
    variants += [(r, c, d) for r in (0, 9, 18, 23, 24, 31) for c in FLAGS + list(range(L.PREV, L.PREV + 100)) for d in (1, P - 1)]
    hit = set()
    for lo in range(0, len(variants), 2500):
        chunk = variants[lo: lo + 2500]
        m = len(chunk)
        loc, nxt = np.empty((L.WIDTH, 2 * m), dtype=np.uint64), np.empty((L.WIDTH, 2 * m), dtype=np.uint64)
        at = np.empty(2 * m, dtype=np.int64)
        for j, (r, c, delta) in enumerate(chunk):            # pair 2 j: row r - 1 with the changed row after it; pair 2 j + 1: the changed row
            changed = rows[r].copy()
            changed[c] = (int(changed[c]) + delta) % P
            loc[:, 2 * j], nxt[:, 2 * j], at[2 * j] = rows[(r - 1) % n_rows], changed, (r - 1) % n_rows
            loc[:, 2 * j + 1], nxt[:, 2 * j + 1], at[2 * j + 1] = changed, rows[(r + 1) % n_rows], r
        fails = CR.eval_pairs(air, loc, nxt, at == 0, at == n_rows - 1)
        assert not fails[:, N_MAIN:].any()
        for j, (r, c, delta) in enumerate(chunk):
            both = np.flatnonzero(fails[2 * j] | fails[2 * j + 1])
            assert both.size > 0, (r, c, delta)
            hit |= set(both.tolist())
    assert sorted(set(range(N_MAIN)) - hit) == []


# ------------------------------------------------------------------------------------------------ 3. proofs
def set_v(table, row, lanes):
    """V of one row := lanes, with the columns that restate it on the same row (MB, XR)"""
    table[row, L.V: L.V + 100] = K.limbs_of(lanes)[0]
    table[row, L.MB: L.MB + 1088] = ((lanes[:17, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(-1)
    table[row, L.XR: L.XR + 68] = K.limbs_of(lanes ^ R.lanes_at(table, row, L.PREV))[0][:68]


def test_statement_binds_the_claims():
    msgs = [b"ab", bytes(136)]
    digs = [keccak.keccak256(m) for m in msgs]
    init, claims = S.statement(msgs, digs)
    assert [(b, s, t.shape) for b, s, t in claims] == [(19, -1, (3, 36)), (20, -1, (3, 36)), (21, -1, (2, 18))]
    canon = p3.from_mont(init).tolist()
    assert canon[:3] == [2, 1, 2] and len(canon) == 3 + 2 * 3 * 36 + 2 * 18
    assert canon[3:] == [int(v) for _b, _s, t in claims for v in p3.from_mont(t).reshape(-1)]
    assert p3.from_mont(claims[0][2])[:, :3].tolist() == [[0, 0, 0x6261], [1, 0, 0], [1, 1, 1]]       # (message, block, first limb)
    assert p3.from_mont(claims[1][2])[0, -1] == 0x8000 and p3.from_mont(claims[0][2])[0, 3] == 0x0001  # the verifier pads
    assert p3.from_mont(claims[2][2])[:, :2].tolist() == [[0, 1], [1, 2]]
    assert p3.from_mont(claims[2][2])[1, 2:].astype("<u2").tobytes() == digs[1]
    with pytest.raises(ValueError):
        S.statement(msgs, digs[:1])


def test_proof_level_refusals():
    over = dict(queries=4, pow_bits=2)
    PR.p2_tables(1)              # read once through the oracle, which that resets: before the parameters are set
    o.oracle_set_params(1, **over)
    try:
        blob = hal.make_params(1, **over)
        sponge_air, chip_air = S.keccak_sponge_air(blob), K.keccak_chip_air(blob)
        rng = np.random.default_rng(8)
        msgs = [rng.integers(0, 256, size=150, dtype=np.uint8).tobytes(), b"raiko"]     # two blocks, one block
        digs = [keccak.keccak256(m) for m in msgs]
        honest = R.sponge_rows(msgs)
        ins, outs = R.states_of(honest, 3)
        chip = CR.chip_rows(ins)
        assert honest.shape[0] == 16 and chip.shape[0] == 128 and np.array_equal(CR.outputs_of(chip, 3), outs)
        init, claims = S.statement(msgs, digs)

        def prove(sponge_rows, chip_rows=chip):
            tabs = [p3.Table.from_canonical(sponge_air, sponge_rows), p3.Table.from_canonical(chip_air, chip_rows)]
            return tabs, o.oracle_p3_prove(tabs, init)

        canon = [p3.from_mont(t).astype(np.uint64) for _b, _s, t in claims]

        def as_claims(tuples):
            return [(19 + j, -1, p3.to_mont(t)) for j, t in enumerate(tuples)]

        def with_digest0(lanes):
            """the honest claims but for message 0's digest: the first four of `lanes`"""
            return S.statement(msgs, [lanes[:4].astype("<u8").tobytes(), digs[1]])[1]

        def verdict(sponge_rows, chip_rows=chip, cl=claims):
            """the library's verifier with the claims `cl`.  Beside it the exact-integer claim sum of
            tests/p3_ref_claims.py, which must agree on reason 8, and the oracle's verifier: it knows no claims, the sends
            on bus + 4 .. bus + 6 stay unanswered for it, and like the library's it compares the sums first -- 8 always"""
            tabs, pf = prove(sponge_rows, chip_rows)
            a = p3.verify(tabs, pf, init, params=blob, claims=cl)
            assert o.oracle_p3_verify(tabs, pf, init) == 8 == p3.verify(tabs, pf, init, params=blob)
            ref = [(bus, s, p3.from_mont(t).astype(np.int64).tolist()) for bus, s, t in cl]
            assert RC.accepts(1, tabs, init, pf, ref) == (a != 8)
            return a

        tabs, proof = prove(honest)
        assert S.verify_keccak256(msgs, digs, proof, params=blob) == 0 == verdict(honest)
        # ---- forged statements: the proof is honest, the verifier's messages / digests are not
        other = [msgs[0][:70] + bytes([msgs[0][70] ^ 1]) + msgs[0][71:], msgs[1]]
        assert S.verify_keccak256(other, digs, proof, params=blob) == 8
        wrong = [digs[0], digs[1][:31] + bytes([digs[1][31] ^ 0x80])]
        assert S.verify_keccak256(msgs, wrong, proof, params=blob) == 8
        assert p3.verify(tabs, proof, init, params=blob) == 8 == p3.verify(tabs, proof, init, params=blob, claims=[])    # no claims
        assert p3.verify(tabs, proof, init, params=blob, claims=claims[:2]) == 8
        bad_init = p3.from_mont(init).astype(np.uint64)
        bad_init[1] += 1                                       # another block count for message 0
        assert p3.verify(tabs, proof, p3.to_mont(bad_init), params=blob, claims=claims) != 0
        # ---- forged witnesses.  The verifier compares the cumulative sums before it evaluates the constraints, so a
        # witness whose sends no longer match the claims is refused with 8 whatever else is wrong with it.  Each forgery
        # below is therefore carried through -- the chip's rows and the claims are what the forger would want them to
        # be, every tuple answered -- and the ONE thing left against it is the constraint it breaks: reason 3
        restart = honest.copy()                                # block 1 of message 0 starts from the zero state: the
        restart[3:6, L.PREV: L.PREV + 100] = 0                 # digest claimed for message 0 is that of its last block alone
        restart[3:6, L.PB: L.PB + 1088] = 0
        fresh = R.lanes_at(honest, 3)
        for r, lanes in ((3, fresh), (4, fresh), (5, R.f1600(fresh))):
            set_v(restart, r, lanes)
        assert {r for r, _ in CR.eval_rows(sponge_air, restart)} == {2}
        forged_chip = CR.chip_rows(np.stack([ins[0], fresh, ins[2]]))
        assert verdict(restart, forged_chip, with_digest0(R.f1600(fresh))) == 3
        assert verdict(restart, forged_chip) == 8              # against the honest digest: the sums differ first
        cap = honest.copy()                                    # a capacity limb changes between O and the next group
        cap[3:6, L.PREV + 99] ^= 1
        cap[4, L.V + 99] ^= 1
        forged_in = ins.copy()
        forged_in[1] = R.lanes_at(cap, 4)
        set_v(cap, 5, R.f1600(forged_in[1]))
        assert {r for r, _ in CR.eval_rows(sponge_air, cap)} == {2}
        assert verdict(cap, CR.chip_rows(forged_in), with_digest0(R.f1600(forged_in[1]))) == 3
        withheld = honest.copy()                               # a real X row sends no block: block 1 of message 0 is free
        withheld[3, L.S_MSG] = 0
        assert verdict(withheld, chip, as_claims([np.delete(canon[0], 1, axis=0), np.delete(canon[1], 1, axis=0), canon[2]])) == 3
        assert verdict(withheld) == 8
        shared = honest.copy()                                 # groups 0 and 1 under one PID with their outputs swapped: the
        shared[3:6, L.PID] = 0                                 # chip, its IDs changed alike, still answers every tuple
        set_v(shared, 2, outs[1])
        set_v(shared, 5, outs[0])
        same_id = CR.chip_rows(ins, ids=[0, 0, 2])
        assert CR.eval_rows(chip_air, same_id) == [] and {r for r, _ in CR.eval_rows(sponge_air, shared)} == {2, 5}
        assert verdict(shared, same_id, with_digest0(outs[0])) == 3
        unswapped = honest.copy()                              # one PID alone, nothing swapped: PID must count
        unswapped[3:6, L.PID] = 0
        assert {r for r, _ in CR.eval_rows(sponge_air, unswapped)} == {2, 5} and verdict(unswapped, same_id) == 3
        # a digest sent from block 0 of the two-block message, against the honest claims: 8.  The extra send has no
        # receiver, and the sums are compared first.  With a claim that takes it, what is left is S_DIG = KO LAST: 3.
        # A witness that also sets LAST there, and all that follows from it, is a valid witness of ANOTHER statement --
        # three one-block messages --, which the honest claims do not match: 8
        early = honest.copy()
        early[2, L.S_DIG] = 1
        assert verdict(early) == 8
        extra = np.concatenate([[0, 1], K.limbs_of(outs[0])[0][:16]]).astype(np.uint64)
        assert verdict(early, chip, as_claims([canon[0], canon[1], np.vstack([canon[2], extra])])) == 3
        three = R.sponge_rows([msgs[0][:100], msgs[0][100:], msgs[1]])
        assert three.shape == honest.shape and CR.eval_rows(sponge_air, three) == []
        assert verdict(three, CR.chip_rows(R.states_of(three, 3)[0])) == 8
        stuck = honest.copy()                                  # BLK does not rise: message 0 is claimed as two blocks 0
        stuck[3:6, L.BLK] = 0
        stuck[3:6, L.NBLK] = 1
        low = [c.copy() for c in canon]
        low[0][1, 1] = low[1][1, 1] = 0
        low[2][0, 1] = 1
        assert verdict(stuck, chip, as_claims(low)) == 3 and verdict(stuck) == 8
        again = honest.copy()                                  # REAL rises again: a real group after a padding group, the
        again[12:15] = honest[6:9]                             # chip with a fourth permutation, message 1 claimed twice
        again[12:15, L.PID] = 3
        assert {r for r, _ in CR.eval_rows(sponge_air, again)} == {11}
        twice = as_claims([np.vstack([c, c[-1:]]) for c in canon])
        assert verdict(again, CR.chip_rows(np.vstack([ins, ins[2:]])), twice) == 3
    finally:
        o.oracle_set_params()


# ------------------------------------------------------------------------------------------------ 4. the lane body under g++
@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_keccak_sponge") / "libemul_keccak_sponge.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", "emul_keccak_sponge.cpp")], check=True, capture_output=True)
    lib = C.CDLL(so)
    lib.emul_keccak_sponge_width.restype = C.c_uint32
    lib.emul_keccak_sponge_rows.restype = None
    lib.emul_keccak_sponge_rows.argtypes = [C.c_void_p] * 5 + [C.c_size_t] * 3 + [C.c_void_p]
    return lib


CASES = R.kernel_cases(S.WAVES_PER_BLOCK, S.CHAIN_WAVES_PER_BLOCK)


@pytest.mark.parametrize("name", list(CASES))
def test_lane_body_writes_the_restatement(emul_lib, name):
    msgs, ids, rows = CASES[name]
    assert emul_lib.emul_keccak_sponge_width() == L.WIDTH
    blocks, first = S.pad_blocks(msgs)
    chains = [R.chain(m) for m in msgs]
    ins, outs = (np.ascontiguousarray(np.concatenate([c[j] for c in chains])) for j in (1, 2))
    rows = S.min_rows(blocks.shape[0]) if rows is None else rows
    im = None if ids is None else p3.to_mont(ids)
    trace = np.full((rows, L.WIDTH), 0xFFFFFFFF, dtype=np.uint32)
    emul_lib.emul_keccak_sponge_rows(blocks.ctypes.data, first.ctypes.data, None if im is None else im.ctypes.data, ins.ctypes.data,
                                     outs.ctypes.data, len(msgs), blocks.shape[0], rows, trace.ctypes.data)
    assert np.array_equal(trace, p3.to_mont(R.sponge_rows(msgs, ids, rows)))


def test_lane_body_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = str(tmp_path / "keccak_sponge_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "asan", "keccak_sponge_main.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "keccak_sponge_main ok" in r.stdout


def test_entry_points_refuse_malformed_arguments():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rk_keccak_sponge_air(None, 15, None) == -1
    assert lib.rk_keccak_sponge_air(None, P - 6, C.byref(h)) == -1          # bus + 6 not canonical
    assert lib.rk_keccak_sponge_air(None, P - 7, C.byref(h)) == 0
    lib.rk_air_destroy(h)
    bad = hal.make_params(1)
    bad.p2_width = 20
    assert lib.rk_keccak_sponge_air(C.byref(bad), 15, C.byref(h)) == -1
    assert lib.rk_keccak_sponge_trace(None, None, None, None, 1, 1, 4, None, None, None, None) == -1
