"""TEST INFRASTRUCTURE for the Keccak-256 sponge table (rk_keccak_sponge_air / rk_keccak_sponge_trace,
include/raiko_hip.h): `sponge_rows`, a numpy restatement of the table written from the column definitions -- the
permutation is raiko_amd.keccak._f1600, the padding raiko_amd.keccak.keccak256's --, and what the tests read off it.
The step-list evaluator is tests/keccak_chip_ref.py's (eval_pairs / eval_rows work on any Air)."""
import numpy as np

from raiko_amd import keccak
from raiko_amd.keccak_chip import lanes_of, limbs_of
from raiko_amd.keccak_sponge import RATE, Layout as L, min_rows


def f1600(lanes):
    a = [[int(lanes[x + 5 * y]) for y in range(5)] for x in range(5)]
    return lanes_of(keccak._f1600(a))


def padded(message):
    """Keccak-256's padding -> (n, 17) uint64"""
    b = bytearray(message) + b"\x01"
    while len(b) % RATE:
        b.append(0)
    b[-1] |= 0x80
    return np.frombuffer(bytes(b), dtype="<u8").reshape(-1, 17).astype(np.uint64)


def chain(message):
    """-> (blocks (n, 17), inputs (n, 25), outputs (n, 25)) of the message's permutations, chained by hand"""
    blocks = padded(message)
    state = np.zeros(25, dtype=np.uint64)
    ins, outs = [], []
    for blk in blocks:
        state = state.copy()
        state[:17] ^= blk
        ins.append(state)
        state = f1600(state)
        outs.append(state)
    return blocks, np.array(ins), np.array(outs)


def _bits(v):
    return (v[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)


def sponge_rows(messages, msg_ids=None, rows=None):
    """byte strings, msg_ids canonical (None: 0 .. k - 1) -> (rows, width) canonical uint64; rows past the blocks' are zero"""
    chains = [chain(m) for m in messages]
    nb = sum(c[0].shape[0] for c in chains)
    rows = min_rows(nb) if rows is None else rows
    assert rows >= 3 * nb
    out = np.zeros((rows, L.WIDTH), dtype=np.uint64)
    pid = 0
    for k, (blocks, ins, outs) in enumerate(chains):
        n = blocks.shape[0]
        for b in range(n):
            prev = outs[b - 1] if b else np.zeros(25, dtype=np.uint64)
            x = np.zeros(25, dtype=np.uint64)
            x[:17] = blocks[b]
            for r, v in enumerate((x, ins[b], outs[b])):
                row = out[3 * pid + r]
                row[L.V: L.V + 100] = limbs_of(v)[0]
                row[L.PREV: L.PREV + 100] = limbs_of(prev)[0]
                row[L.MB: L.MB + 1088] = _bits(v[:17]).reshape(-1)
                row[L.PB: L.PB + 1088] = _bits(prev[:17]).reshape(-1)
                row[L.XR: L.XR + 68] = limbs_of(v ^ prev)[0][:68]
                row[L.MSG] = k if msg_ids is None else int(msg_ids[k])
                row[L.BLK], row[L.NBLK], row[L.PID] = b, b + 1, pid
                row[L.KX + r] = row[L.REAL] = 1
                row[L.FIRST], row[L.LAST] = b == 0, b == n - 1
                row[(L.S_MSG, L.S_IN, L.S_OUT)[r]] = 1
                row[L.S_DIG] = r == 2 and b == n - 1
            pid += 1
    return out


def set_12131(seed=12131):
    """five messages of 1, 2, 1, 3, 1 blocks (135 bytes still fit one block, 136 need two), random bytes"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=n, dtype=np.uint8).tobytes() for n in (10, 200, 135, 300, 0)]


def kernel_cases(rows_waves, chain_waves):
    """name -> (messages, msg_ids canonical or None, rows or None): the smallest shapes at which the two kernels can go
    wrong.  rows_waves / chain_waves: block slots / messages per thread block of the rows / the chain kernel"""
    rng = np.random.default_rng(256)
    msg = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    return {
        "empty": ([b""], None, None),
        "135 bytes, pad byte 0x81": ([msg(135)], None, None),
        "136 bytes, a block of padding": ([msg(136)], None, None),
        "137 bytes": ([msg(137)], None, None),
        "1, 2, 1, 3, 1 blocks": (set_12131(), None, None),
        "one full block of the rows kernel": ([msg(20 + i) for i in range(rows_waves)], None, None),
        "the first second block of the rows kernel": ([msg(30 + i) for i in range(rows_waves + 1)], None, None),
        "one full block of the chain kernel": ([msg(136 * (i % 2) + 7 * i) for i in range(chain_waves)], None, None),
        "the first second block of the chain kernel": ([msg(136 * ((i + 1) % 2) + 5 * i) for i in range(chain_waves + 1)], None, None),
        "nine blocks": ([msg(8 * 136 + 5)], None, None),
        "half the slots padding": (set_12131(7), None, 64),
        "given msg_ids": ([msg(3), msg(140), msg(0)], [7, P_MINUS_1, 123456], None),
    }


P_MINUS_1 = 2013265920


def lanes_at(table, row, col=L.V):
    limbs = np.asarray(table[row, col: col + 100], dtype=np.uint64).reshape(25, 4)
    return limbs[:, 0] | limbs[:, 1] << np.uint64(16) | limbs[:, 2] << np.uint64(32) | limbs[:, 3] << np.uint64(48)


def states_of(table, n_blocks):
    """(inputs, outputs) (n_blocks, 25) uint64: V of the I rows and of the O rows"""
    return (np.stack([lanes_at(table, 3 * b + 1) for b in range(n_blocks)]), np.stack([lanes_at(table, 3 * b + 2) for b in range(n_blocks)]))


def digests_of(table):
    """the digests the table sends: the first four lanes of V on the rows with S_DIG, as 32-byte strings"""
    return [lanes_at(table, r)[:4].astype("<u8").tobytes() for r in np.flatnonzero(table[:, L.S_DIG])]
