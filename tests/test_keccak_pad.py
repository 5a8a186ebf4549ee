"""The Keccak-256 padding table (rk_keccak_pad_air / rk_keccak_pad_trace, include/raiko_hip.h; raiko_amd/keccak_pad.py)
on the CPU: the numpy restatement of its table (tests/keccak_pad_ref.py) places the padded blocks of
keccak_sponge.pad_blocks whatever stands past a message's end; the library-written AIR accepts it and pins every
committed cell; the oracle proves [pad, sponge, chip], the verifier adds the receive claims of ITS words, lengths and
digests, and forged statements and forged witnesses are refused; the kernel bodies, run under g++ (and once more as a
program of its own under AddressSanitizer and UBSan), write blocks and table word for word.  Everything is bit-exact."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import keccak_chip_ref as CR
import keccak_pad_ref as R
import keccak_sponge_ref as SR
import oracle_lib as o
import p3_ref as PR
import p3_ref_claims as RC
from raiko_amd import _lib, hal, keccak, keccak_chip as K, keccak_pad as KP, keccak_sponge as S, p3

P = o.P
L = KP.Layout
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_MAIN = 378 - 24            # the lookup argument's own 24: three batches x 4, first / transition / last 3 x 4
D_COLS = list(range(L.D, L.D + 16))
FIVE_TAIL = [b"\x11\x22", b"", b"\x33", b"", b""]


@pytest.fixture(scope="module")
def air():
    return KP.keccak_pad_air()


@pytest.fixture(scope="module")
def five():
    """the (1, 2, 1, 3, 1) set, 10 / 200 / 135 / 300 / 0 bytes: 272 real rows of 512"""
    msgs = SR.set_12131()
    rows = R.pad_rows(msgs, tail=FIVE_TAIL)
    rows.setflags(write=False)
    return msgs, rows


# ------------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("garbage", [False, True])
def test_the_restatement_places_pad_blocks(garbage):
    rng = np.random.default_rng(1001)
    for n in (0, 1, 3, 4, 5, 131, 132, 133, 134, 135, 136, 137, 271, 272, 273, 1000):
        m = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        tail = [rng.integers(1, 256, size=3, dtype=np.uint8).tobytes()] if garbage else None
        rows = R.pad_rows([m], tail=tail)
        blocks, first = S.pad_blocks([m])
        assert np.array_equal(R.blocks_of(rows), blocks) and rows.shape[0] == KP.min_rows(first[-1]), n
        n_real = 34 * int(first[-1])
        assert rows[:n_real, L.REAL].all() and not rows[n_real:].any()
        assert int(rows[:, L.R].sum()) == -(-n // 4) and int(rows[:, L.END].sum()) == 1 == int(rows[:, L.S_END].sum())
        assert rows[n_real - 1, L.S_END] == 1 and rows[n_real - 1, L.D: L.D + 16].astype("<u2").tobytes() == keccak.keccak256(m)
        words, word_first, lens, first2 = KP.words_of([m], tail)
        assert np.array_equal(first2, first) and lens.tolist() == [n] and word_first.tolist() == [0, -(-n // 4)]
        sent = rows[rows[:, L.R] == 1]
        assert np.array_equal(sent[:, L.W_LO] | sent[:, L.W_HI] << np.uint64(16), words) and sent[:, L.IDX].tolist() == list(range(words.size))
        if garbage and n % 4:                       # the garbage stands in the word handed over and nowhere in the block
            assert words[-1] >> (8 * (n % 4)) != 0


# ------------------------------------------------------------------------------------------------ 2. the AIR
def test_air_shape(air):
    lib = _lib.load()
    info = air.info()
    assert info["max_degree"] <= 3 and info["log_quotient_degree"] == 1 == air.log_quotient_degree()
    assert air.width == L.WIDTH == int(lib.rk_keccak_pad_width()) and int(lib.rk_keccak_pad_rows_per_block()) == KP.ROWS_PER_BLOCK == 34
    assert info["n_constraints"] == air.n_constraints == N_MAIN + 24
    its = air.interactions
    assert [it.bus for it in its] == [19, 20, 21, 22, 23] and K.BUS_KECCAK == 15
    assert [it.kind for it in its] == [p3.RECEIVE] * 3 + [p3.SEND] * 2 and not any(it.mult_is_const for it in its)
    assert [it.mult for it in its] == [L.STEP + 33, L.STEP + 33, L.S_END, L.R, L.S_END]
    assert [len(it.value_cols) for it in its] == [36, 36, 18, 4, 18] and max(len(it.value_cols) for it in its) <= 64
    assert len({c for it in its for c in it.value_cols + [it.mult]}) == 94 <= 120
    sponge = S.keccak_sponge_air()                   # the receives take what the sponge's last three send, tuple for tuple
    assert [(it.bus, len(it.value_cols)) for it in sponge.interactions[4:]] == [(it.bus, len(it.value_cols)) for it in its[:3]]
    assert its[0].value_cols == [L.MSG, L.BLK] + list(range(34)) and its[1].value_cols == [L.MSG, L.BLK] + list(range(34, 68))
    assert its[2].value_cols == [L.MSG, L.NBLK] + D_COLS and its[4].value_cols == [L.MSG, L.LEN] + D_COLS
    assert its[3].value_cols == [L.MSG, L.IDX, L.W_LO, L.W_HI]
    other = KP.keccak_pad_air(hal.make_params(0), bus=30)         # risc0's extension: the same main constraints
    n_main = int(np.flatnonzero(air.steps[:, 0] == p3.ASSERT_ZERO)[N_MAIN - 1]) + 1
    assert np.array_equal(other.steps[:n_main], air.steps[:n_main]) and not np.array_equal(other.steps, air.steps)
    assert [it.bus for it in other.interactions] == list(range(34, 39))


def test_python_restates_the_layout_and_the_launch_constants():
    hpp = open(os.path.join(ROOT, "raiko_amd", "csrc", "keccak_pad.hpp")).read()
    hip = open(os.path.join(ROOT, "raiko_amd", "csrc", "keccak_pad.hip")).read()
    assert int(re.search(r"constexpr unsigned KP_WAVES = (\d+);", hip).group(1)) == KP.ROWS_WAVES_PER_BLOCK
    assert int(re.search(r"constexpr unsigned KP_BLOCKS_THREADS = (\d+);", hip).group(1)) == KP.BLOCKS_THREADS
    named = dict(re.findall(r"\b([A-Z_]+) = (\d+)[,;]", hpp[hpp.index("struct KeccakPadLayout"): hpp.index("// ---- the padded blocks")]))
    for name in ("W_LO", "W_HI", "MSG", "BLK", "NBLK", "IDX", "LEN", "DATA", "END", "AFTER", "REAL", "R", "S_END", "WIDTH"):
        assert int(named[name]) == getattr(L, name), name
    assert int(named["ROWS"]) == KP.ROWS_PER_BLOCK and int(named["BLOCK_LIMBS"]) * 2 == S.RATE
    for fn, at in (("b", L.B), ("step", L.STEP), ("wb", L.WB), ("e", L.E), ("d", L.D)):
        assert int(re.search(r"uint32_t %s\([^)]*\) \{ return (\d+)? ?\+? ?" % fn, hpp).group(1) or 0) == at, fn


@pytest.mark.parametrize("case", ["empty", "five", "twice"])
def test_air_accepts_the_restatement(air, five, case):
    table = {"empty": lambda: R.pad_rows([b""]), "five": lambda: five[1], "twice": lambda: R.pad_rows(five[0], rows=1024, tail=FIVE_TAIL)}[case]()
    assert table.shape[0] == {"empty": 64, "five": 512, "twice": 1024}[case]
    assert air.check_trace(table) == [] == CR.eval_rows(air, table)
    n_real = int(table[:, L.REAL].sum())
    assert n_real % 34 == 0 and table[:n_real, L.REAL].all() and not table[n_real:].any()       # real blocks, then zero rows


def test_every_committed_cell_is_pinned(air, five):
    """One cell changed by + 1 or - 1: some main-trace constraint fails at the row before or at the row itself; between
    them the variants reach every constraint.  Constraints read a row and its successor only, so those two pairs are all
    that is evaluated, batched over the variants.  The one exception is D on a message's last row: there the sponge's send
    on bus + 6 is what binds it, not a constraint -- test_proof_level_refusals changes such a cell and meets reason 8."""
    _msgs, rows = five
    n_rows = rows.shape[0]
    # messages at rows 0 (10 bytes), 34 (200), 102 (135), 136 (300), 238 (0); padding from 272.  Every column of: a DATA
    # row (40), an END row with e = 0 (84), the END row with e = 3 on STEP[33] (135: the 135-byte message's last), an AFTER
    # row (90), a STEP[33] row inside a message (67), a padding row (300); on top the rows where only a special place
    # reaches a constraint: the table's first (0), an END row with e = 2 (2), a message's last row (33), a message's first
    # (34), a block's first inside a message (68), the last real row (271), the first padding row (272), the table's last (511)
    assert rows[40, L.DATA] == rows[84, L.END] == rows[84, L.E] == rows[135, L.END] == rows[135, L.E + 3] == rows[135, L.STEP + 33] == 1
    assert rows[90, L.AFTER] == rows[67, L.STEP + 33] == rows[67, L.DATA] == rows[2, L.E + 2] == rows[33, L.S_END] == rows[68, L.STEP] == 1
    assert rows[135, L.S_END] == rows[271, L.S_END] == 1 and rows[34, L.IDX] == 0 and rows[34, L.MSG] == 1 and not rows[272:].any()
    everywhere = (40, 84, 135, 90, 67, 300, 0, 2, 33, 34, 68, 271, 272, 511)
    variants = [(r, c, d) for r in everywhere for c in range(L.WIDTH) for d in (1, P - 1) if not (rows[r, L.S_END] == 1 and c in D_COLS)]
    free = [(r, c, d) for r in (33, 135, 271) for c in D_COLS for d in (1, P - 1)]
    hit = set()
    for lo in range(0, len(variants) + len(free), 2500):
        chunk = (variants + free)[lo: lo + 2500]
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
            assert (both.size > 0) == (lo + j < len(variants)), (r, c, delta)
            hit |= set(both.tolist())
    assert sorted(set(range(N_MAIN)) - hit) == []


# ------------------------------------------------------------------------------------------------ 3. proofs
def test_statement_words_binds_the_claims():
    msgs = [b"abcde", bytes(136), b""]
    digs = [keccak.keccak256(m) for m in msgs]
    init, claims = KP.statement_words(msgs, digs, tail=[b"\x07\x08\x09", b"", b""])
    assert [(b, s, t.shape) for b, s, t in claims] == [(22, -1, (36, 4)), (23, -1, (3, 18))]
    canon = p3.from_mont(init).tolist()
    assert canon[:4] == [3, 5, 136, 0] and len(canon) == 4 + 36 * 4 + 3 * 18
    assert canon[4:] == [int(v) for _b, _s, t in claims for v in p3.from_mont(t).reshape(-1)]
    assert p3.from_mont(claims[0][2])[:3].tolist() == [[0, 0, 0x6261, 0x6463], [0, 1, 0x0765, 0x0908], [1, 0, 0, 0]]   # no 0x01 anywhere
    assert p3.from_mont(claims[1][2])[:, :2].tolist() == [[0, 5], [1, 136], [2, 0]]
    assert p3.from_mont(claims[1][2])[2, 2:].astype("<u2").tobytes() == digs[2]
    with pytest.raises(ValueError):
        KP.statement_words(msgs, digs[:1])


def test_proof_level_refusals():
    over = dict(queries=4, pow_bits=2)
    PR.p2_tables(1)              # read once through the oracle, which that resets: before the parameters are set
    o.oracle_set_params(1, **over)
    try:
        blob = hal.make_params(1, **over)
        pad_air, sponge_air, chip_air = KP.keccak_pad_air(blob), S.keccak_sponge_air(blob), K.keccak_chip_air(blob)
        rng = np.random.default_rng(9)
        msgs = [rng.integers(0, 256, size=150, dtype=np.uint8).tobytes(), b"raiko", rng.integers(0, 256, size=9, dtype=np.uint8).tobytes()]
        tail = [b"\x5a\x5b", b"\xc3\xc4\xc5", b"\x99\x98\x97"]       # 150 = 4 x 37 + 2, 5 = 4 + 1, 9 = 8 + 1
        digs = [keccak.keccak256(m) for m in msgs]
        honest = R.pad_rows(msgs, tail=tail)                   # message 0 at rows 0 .. 67, 1 at 68 .. 101, 2 at 102 .. 135
        assert honest.shape[0] == 256 and CR.eval_rows(pad_air, honest) == []
        assert honest[37, L.END] == honest[69, L.END] == honest[104, L.END] == 1 and honest[[67, 101, 135], L.S_END].all()

        def as_claims(words, per_msg):
            return [(22, -1, p3.to_mont(words)), (23, -1, p3.to_mont(per_msg))]

        def init_of(words, per_msg):
            return p3.to_mont(np.concatenate([np.array([per_msg.shape[0]], dtype=np.uint64), per_msg[:, 1], words.reshape(-1), per_msg.reshape(-1)]))

        def verdict(pad_rows, claims=None, init=None, expect_sums=None):
            """the forged pad table carried through (tests/keccak_pad_ref.py carry): sponge and chip absorb the blocks it
            receives, D and the claims are what it sends -- unless `claims` are given --, and the library's verifier
            decides.  Beside it the exact-integer claim sum of tests/p3_ref_claims.py, which must agree on reason 8, and
            the oracle's verifier, which knows no claims: 8 always"""
            table, sponge, ins, words, per_msg = R.carry(pad_rows)
            assert CR.eval_rows(sponge_air, sponge) == []
            tabs = [p3.Table.from_canonical(pad_air, table), p3.Table.from_canonical(sponge_air, sponge), p3.Table.from_canonical(chip_air, CR.chip_rows(ins))]
            cl = as_claims(words, per_msg) if claims is None else claims
            iw = init_of(words, per_msg) if init is None else init
            pf = o.oracle_p3_prove(tabs, iw)
            a = p3.verify(tabs, pf, iw, params=blob, claims=cl)
            assert o.oracle_p3_verify(tabs, pf, iw) == 8 == p3.verify(tabs, pf, iw, params=blob)
            ref = [(bus, s, p3.from_mont(t).astype(np.int64).tolist()) for bus, s, t in cl]
            assert RC.accepts(1, tabs, iw, pf, ref) == (a != 8)
            return a, pf

        def broken(pad_rows):
            return {r for r, _ in CR.eval_rows(pad_air, pad_rows)}

        # ---- the honest proof: carried through it is what statement_words forms, and both verifiers accept it
        init, claims = KP.statement_words(msgs, digs, tail=tail)
        table, _sponge, _ins, words, per_msg = R.carry(honest)
        assert np.array_equal(table, honest) and np.array_equal(init_of(words, per_msg), init)
        assert all(np.array_equal(a[2], b[2]) for a, b in zip(as_claims(words, per_msg), claims))
        a, proof = verdict(honest)
        assert a == 0 == KP.verify_keccak256_words(msgs, digs, proof, params=blob, tail=tail)
        # ---- forged statements: the proof is honest, the verifier's words / lengths / digests are not
        flipped = [msgs[0][:70] + bytes([msgs[0][70] ^ 1]) + msgs[0][71:]] + msgs[1:]
        assert KP.verify_keccak256_words(flipped, digs, proof, params=blob, tail=tail) == 8
        garbage = [tail[0], b"\xc3\xc4\xc4", tail[2]]           # a bit of the bytes past the end: another word claim
        assert KP.verify_keccak256_words(msgs, digs, proof, params=blob, tail=garbage) == 8
        # a length changed by one within the same last word, every word claim unchanged: message 1 as 6 bytes (0xc3 taken
        # in), message 0 as 149 (its last byte left out)
        longer = [msgs[0], msgs[1] + tail[1][:1], msgs[2]]
        assert KP.words_of(longer, [tail[0], tail[1][1:], tail[2]])[0].tolist() == KP.words_of(msgs, tail)[0].tolist()
        assert KP.verify_keccak256_words(longer, digs, proof, params=blob, tail=[tail[0], tail[1][1:], tail[2]]) == 8
        shorter = [msgs[0][:-1], msgs[1], msgs[2]]
        assert KP.words_of(shorter, [msgs[0][-1:] + tail[0], tail[1], tail[2]])[0].tolist() == KP.words_of(msgs, tail)[0].tolist()
        assert KP.verify_keccak256_words(shorter, digs, proof, params=blob, tail=[msgs[0][-1:] + tail[0], tail[1], tail[2]]) == 8
        wrong = [digs[0], digs[1][:31] + bytes([digs[1][31] ^ 0x80]), digs[2]]
        assert KP.verify_keccak256_words(msgs, wrong, proof, params=blob, tail=tail) == 8
        tabs = [p3.Table.from_canonical(pad_air, honest), p3.Table.pinned(sponge_air, 4), p3.Table.pinned(chip_air, 7)]
        assert p3.verify(tabs, proof, init, params=blob) == 8 == p3.verify(tabs, proof, init, params=blob, claims=[])    # no claims
        assert p3.verify(tabs, proof, init, params=blob, claims=claims[:1]) == 8
        dropped = [(22, -1, np.delete(claims[0][2], 5, axis=0)), claims[1]]                                             # a word claim dropped
        assert p3.verify(tabs, proof, init, params=blob, claims=dropped) == 8
        bad_init = p3.from_mont(init).astype(np.uint64)
        bad_init[1] += 1                                       # another length for message 0
        assert p3.verify(tabs, proof, p3.to_mont(bad_init), params=blob, claims=claims) != 0
        # D on a message's last row is bound by the sponge's send alone: changed, the sums differ
        d_changed = honest.copy()
        d_changed[101, L.D + 3] += 1
        assert broken(d_changed) == set()
        tabs_d = [p3.Table.from_canonical(pad_air, d_changed), p3.Table.from_canonical(sponge_air, _sponge), p3.Table.from_canonical(chip_air, CR.chip_rows(_ins))]
        pf_d = o.oracle_p3_prove(tabs_d, init)
        changed_digs = [digs[0], d_changed[101, L.D: L.D + 16].astype("<u2").tobytes(), digs[2]]
        assert KP.verify_keccak256_words(msgs, digs, pf_d, params=blob, tail=tail) == 8
        assert KP.verify_keccak256_words(msgs, changed_digs, pf_d, params=blob, tail=tail) == 8
        # ---- forged witnesses.  The verifier compares the cumulative sums before it evaluates the constraints, so a
        # witness whose tuples no longer meet the claims is refused with 8 whatever else is wrong with it.  Each forgery
        # below is therefore carried through -- sponge, chip, D and the claims are what the forger would want them to
        # be, every tuple answered -- and the ONE thing left against it is the constraint it breaks: reason 3
        f = honest.copy()                                      # 0x01 omitted: message 1 hashed as "raiko" 0x00 .. 0x80
        f[69, L.B + 66] -= 0x100
        assert broken(R.propagate(f)) == {69} and verdict(f)[0] == 3
        f = honest.copy()                                      # 0x80 omitted from message 1's block
        f[101, L.B + 67] -= 0x8000
        assert broken(f) == {101} and verdict(f)[0] == 3
        f = honest.copy()                                      # a tail byte let through: message 1's byte 5 is 0xc3, 0x01 after it
        f[69, L.B + 66], f[69, L.B + 67] = honest[69, L.W_LO], 0x01
        assert honest[69, L.W_LO] == 0xc36f and broken(R.propagate(f)) == {69} and verdict(f)[0] == 3
        f = honest.copy()                                      # END one row late in message 2: LEN stays 9, three more bytes hashed
        f[104] = R.message_rows(msgs[2] + tail[2], b"")[2]
        f[105] = R.message_rows(msgs[2] + tail[2] + b"\x00", b"")[3]
        f[104:106, L.MSG], f[104:106, L.LEN], f[105, L.E: L.E + 4], f[105, L.R] = 2, 9, [0, 1, 0, 0], 1
        f[105, L.B + 66] = 0x100
        assert f[104, L.DATA] == f[105, L.END] == 1 and broken(R.propagate(f)) == {105} and verdict(f)[0] == 3
        f = honest.copy()                                      # two END rows in message 2: the second places 0x01 again
        f[105, [L.END, L.AFTER, L.E + 1, L.R]] = [1, 0, 1, 1]
        f[105, L.B + 66] = 0x100
        assert broken(R.propagate(f)) == {104, 105} and verdict(f)[0] == 3
        f = honest.copy()                                      # message 1 ended off a block boundary: a message 3 opens at its row 20
        f[88:102, L.MSG], f[88:102, L.IDX] = 3, np.arange(14)
        f[88:102, L.LEN] = 0
        f[88, [L.END, L.AFTER, L.E]] = [1, 0, 1]
        f[88, L.B + 66] = 1
        assert broken(R.propagate(f)) == {87} and verdict(f)[0] == 3
        f = honest.copy()                                      # IDX does not rise in message 0: claimed four bytes shorter
        f[20:68, L.IDX] -= 1
        f[0:68, L.LEN] -= 4
        assert broken(f) == {19} and verdict(f)[0] == 3
        f = honest.copy()                                      # a withheld R: word 3 of message 0 is hashed and never claimed
        f[3, L.R] = 0
        assert broken(f) == {3} and verdict(f)[0] == 3
        a, _pf = verdict(f, claims=claims, init=init)          # against the honest claims: the sums differ first
        assert a == 8
        f = honest.copy()                                      # REAL rises again: message 1 once more after padding rows
        f[170:204] = honest[68:102]
        f[170:204, L.MSG] = 3
        assert broken(f) == {169} and verdict(f)[0] == 3
    finally:
        o.oracle_set_params()


# ------------------------------------------------------------------------------------------------ 4. the kernel bodies under g++
@pytest.fixture(scope="module")
def emul_lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_keccak_pad") / "libemul_keccak_pad.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", so,
                    os.path.join(ROOT, "tests", "emul", "emul_keccak_pad.cpp")], check=True, capture_output=True)
    lib = C.CDLL(so)
    lib.emul_keccak_pad_width.restype = C.c_uint32
    lib.emul_keccak_pad.restype = None
    lib.emul_keccak_pad.argtypes = [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5 + [C.c_size_t] * 3 + [C.c_void_p] * 2
    return lib


CASES = R.kernel_cases()


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_bodies_write_the_restatement(emul_lib, name):
    msgs, ids, rows, tail = CASES[name]
    assert emul_lib.emul_keccak_pad_width() == L.WIDTH
    words, word_first, lens, first = KP.words_of(msgs, tail)
    nb = int(first[-1])
    rows = KP.min_rows(nb) if rows is None else rows
    im = None if ids is None else p3.to_mont(ids)
    digs = np.frombuffer(b"".join(keccak.keccak256(m) for m in msgs), dtype="<u8").copy()
    for with_digests in (False, True):
        trace = np.full((rows, L.WIDTH), 0xFFFFFFFF, dtype=np.uint32)
        blocks = np.full((nb, 17), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
        buf = words if words.size else np.zeros(1, dtype=np.uint32)
        emul_lib.emul_keccak_pad(buf.ctypes.data, words.size, word_first.ctypes.data, lens.ctypes.data, first.ctypes.data,
                                 None if im is None else im.ctypes.data, digs.ctypes.data if with_digests else None, len(msgs), nb, rows,
                                 trace.ctypes.data, blocks.ctypes.data)
        assert np.array_equal(blocks, S.pad_blocks(msgs)[0])
        assert np.array_equal(trace, p3.to_mont(R.pad_rows(msgs, ids, rows, tail, digests=with_digests)))


def test_kernel_bodies_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = str(tmp_path / "keccak_pad_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "asan", "keccak_pad_main.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "keccak_pad_main ok" in r.stdout


def test_entry_points_refuse_malformed_arguments():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.rk_keccak_pad_air(None, 15, None) == -1
    assert lib.rk_keccak_pad_air(None, P - 8, C.byref(h)) == -1           # bus + 8 not canonical
    assert lib.rk_keccak_pad_air(None, P - 9, C.byref(h)) == 0
    lib.rk_air_destroy(h)
    bad = hal.make_params(1)
    bad.p2_width = 20
    assert lib.rk_keccak_pad_air(C.byref(bad), 15, C.byref(h)) == -1
    assert lib.rk_keccak_pad_trace(None, None, 0, None, None, None, None, 1, 1, 64, None, None) == -1
    assert lib.rk_keccak_pad_digests(None, None, None, 1, 1, 64, None) == -1
