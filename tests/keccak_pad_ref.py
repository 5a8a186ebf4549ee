"""TEST INFRASTRUCTURE for the Keccak-256 padding table (rk_keccak_pad_air / rk_keccak_pad_trace, include/raiko_hip.h):
`pad_rows`, a numpy restatement of the table written from the column definitions -- one Python loop over the word slots,
bytes handled one at a time, no use of raiko_amd.keccak_sponge.pad_blocks --, and what the tests read off it.  The
step-list evaluator is tests/keccak_chip_ref.py's (eval_pairs / eval_rows work on any Air)."""
import numpy as np

from raiko_amd import keccak
from raiko_amd.keccak_pad import BLOCKS_THREADS, ROWS_WAVES_PER_BLOCK, Layout as L, min_rows

P_MINUS_1 = 2013265920


def message_rows(message, tail=b""):
    """one message's rows but for MSG and D: byte string, the bytes past its end in its last word -> (34 n, width)"""
    n_len = len(message)
    q, e = divmod(n_len, 4)
    n_rows = 34 * (q // 34 + 1)                 # through the block that holds the END word
    src = bytes(message) + (bytes(tail) + bytes(3))[: -n_len % 4]
    out = np.zeros((n_rows, L.WIDTH), dtype=np.uint64)
    placed = []
    for idx in range(n_rows):
        row, t = out[idx], idx % 34
        data, end = idx < q, idx == q
        takes = data or (end and e != 0)
        w = int.from_bytes(src[4 * idx: 4 * idx + 4], "little") if takes else 0
        by = [(w >> (8 * n)) & 0xFF for n in range(4)]
        if data:
            kept = by
        elif end:
            kept = by[:e] + [0x01] + [0] * (3 - e)
        else:
            kept = [0, 0, 0, 0]
        last = t == 33 and not data
        if last:
            kept = kept[:3] + [kept[3] + 0x80]
        placed.append(kept[0] | kept[1] << 8 | kept[2] << 16 | kept[3] << 24)
        for j in range(68):                     # B[j] on the row of word t: limb j + 2 t - 66 of the block so far
            at = j + 2 * t - 66
            if at >= 0:
                row[L.B + j] = (placed[idx - t + at // 2] >> (16 * (at & 1))) & 0xFFFF
        row[L.STEP + t] = 1
        row[L.W_LO], row[L.W_HI] = w & 0xFFFF, w >> 16
        row[L.WB: L.WB + 32] = [(w >> z) & 1 for z in range(32)]
        if end:
            row[L.E + e] = 1
        row[L.BLK], row[L.NBLK], row[L.IDX], row[L.LEN] = idx // 34, idx // 34 + 1, idx, n_len
        row[L.DATA], row[L.END], row[L.AFTER], row[L.REAL] = data, end, not data and not end, 1
        row[L.R], row[L.S_END] = takes, last
    return out


def pad_rows(messages, msg_ids=None, rows=None, tail=None, digests=True):
    """byte strings, msg_ids canonical (None: 0 .. k - 1) -> (rows, width) canonical uint64; rows past the blocks' are
    zero.  digests: D holds Keccak-256 of each message on its last row (False: 0, as before rk_keccak_pad_digests)"""
    parts = []
    for k, m in enumerate(messages):
        part = message_rows(m, b"" if tail is None else tail[k])
        part[:, L.MSG] = k if msg_ids is None else int(msg_ids[k])
        if digests:
            part[-1, L.D: L.D + 16] = np.frombuffer(keccak.keccak256(bytes(m)), dtype="<u2")
        parts.append(part)
    real = np.concatenate(parts)
    rows = min_rows(real.shape[0] // 34) if rows is None else rows
    assert rows >= real.shape[0]
    out = np.zeros((rows, L.WIDTH), dtype=np.uint64)
    out[: real.shape[0]] = real
    return out


def blocks_of(table):
    """the padded blocks the table receives: B of the STEP[33] rows -> (n_blocks, 17) uint64"""
    limbs = np.asarray(table[table[:, L.STEP + 33] == 1, L.B: L.B + 68], dtype=np.uint64).reshape(-1, 17, 4)
    return limbs[..., 0] | limbs[..., 1] << np.uint64(16) | limbs[..., 2] << np.uint64(32) | limbs[..., 3] << np.uint64(48)


def set_12131():
    import keccak_sponge_ref
    return keccak_sponge_ref.set_12131()


def kernel_cases():
    """name -> (messages, msg_ids canonical or None, rows or None, tail or None): the smallest shapes at which the
    kernels can go wrong.  A thread block of the rows kernel takes ROWS_WAVES_PER_BLOCK block slots, one of the
    blocks kernel BLOCKS_THREADS word slots, 34 a block"""
    rng = np.random.default_rng(257)
    msg = lambda n: rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    full = BLOCKS_THREADS // 34
    return {
        "empty": ([b""], None, None, None),
        "3 bytes, a tail": ([msg(3)], None, None, [b"\xa5"]),
        "135 bytes, pad byte 0x81": ([msg(135)], None, None, [b"\xff"]),
        "136 bytes, a block of padding": ([msg(136)], None, None, None),
        "137 bytes": ([msg(137)], None, None, [b"\x01\x80\xff"]),
        "1, 2, 1, 3, 1 blocks": (set_12131(), None, None, [b"\x11\x22", b"", b"\x33", b"", b""]),
        "one full block of the rows kernel": ([msg(20 + i) for i in range(ROWS_WAVES_PER_BLOCK)], None, None, None),
        "the first second block of the rows kernel": ([msg(30 + i) for i in range(ROWS_WAVES_PER_BLOCK + 1)], None, None, None),
        "one full block of the blocks kernel": ([msg(40 + 9 * i) for i in range(full)], None, None, None),
        "the first second block of the blocks kernel": ([msg(50 + 7 * i) for i in range(full + 1)], None, None, None),
        "nine blocks": ([msg(8 * 136 + 5)], None, None, [b"\x77\x88\x99"]),
        "half the slots padding": (set_12131(), None, 1024, None),
        "given msg_ids": ([msg(3), msg(140), msg(0)], [7, P_MINUS_1, 123456], None, None),
    }


# ------------------------------------------------------------------------------------------------ carrying a pad table through
def propagate(table):
    """B[0..65] of every real row rewritten from the placed words B[66], B[67] of the rows before it in its block: what a
    forger who changes a placed word has to do to keep the shift register's constraints"""
    for r in np.flatnonzero(table[:, L.REAL] == 1):
        t = int(np.flatnonzero(table[r, L.STEP: L.STEP + 34])[0])
        for j in range(66):
            at = j + 2 * t - 66
            table[r, L.B + j] = table[r - t + at // 2, L.B + 66 + (at & 1)] if at >= 0 else 0
    return table


def sponge_rows_of_blocks(groups, rows=None):
    """[(message id, blocks (n, 17) uint64)] -> the sponge table (tests/keccak_sponge_ref.py sponge_rows) that absorbs
    these blocks AS THEY ARE, whatever their padding, and the permutations' inputs (n_blocks, 25)"""
    import keccak_sponge_ref as SR
    from raiko_amd.keccak_chip import limbs_of
    from raiko_amd.keccak_sponge import Layout as SL, min_rows as sponge_min_rows
    nb = sum(b.shape[0] for _i, b in groups)
    out = np.zeros((sponge_min_rows(nb) if rows is None else rows, SL.WIDTH), dtype=np.uint64)
    bits = lambda v: ((v[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(-1)
    pid, ins = 0, []
    for msg, blocks in groups:
        state = np.zeros(25, dtype=np.uint64)
        for b, blk in enumerate(blocks):
            prev = state
            x = np.zeros(25, dtype=np.uint64)
            x[:17] = blk
            inp = prev ^ x
            state = SR.f1600(inp)
            ins.append(inp)
            for r, v in enumerate((x, inp, state)):
                row = out[3 * pid + r]
                row[SL.V: SL.V + 100], row[SL.PREV: SL.PREV + 100] = limbs_of(v)[0], limbs_of(prev)[0]
                row[SL.MB: SL.MB + 1088], row[SL.PB: SL.PB + 1088] = bits(v[:17]), bits(prev[:17])
                row[SL.XR: SL.XR + 68] = limbs_of(v ^ prev)[0][:68]
                row[SL.MSG], row[SL.BLK], row[SL.NBLK], row[SL.PID] = msg, b, b + 1, pid
                row[SL.KX + r] = row[SL.REAL] = 1
                row[SL.FIRST], row[SL.LAST] = b == 0, b == len(blocks) - 1
                row[(SL.S_MSG, SL.S_IN, SL.S_OUT)[r]] = 1
                row[SL.S_DIG] = r == 2 and b == len(blocks) - 1
            pid += 1
    return out, np.array(ins)


def carry(table):
    """a pad table, honest or forged -> (the table with D set, sponge rows, permutation inputs, word tuples, message
    tuples): everything around it as a forger would want it.  The sponge absorbs the blocks the table receives, one
    sponge message per S_END row with that row's MSG; D and the claimed digests are what comes out; the claims are the
    tuples the table sends.  The table's own BLK / NBLK must count the blocks of each group, or the sums cannot meet"""
    from raiko_amd.keccak_sponge import Layout as SL
    table = table.copy()
    blocks, at = blocks_of(table), np.flatnonzero(table[:, L.STEP + 33] == 1)
    groups, lo = [], 0
    for i, r in enumerate(at):
        if table[r, L.S_END] == 1:
            groups.append((int(table[r, L.MSG]), blocks[lo: i + 1]))
            lo = i + 1
    assert lo == len(at), "blocks after the last message end"
    sponge, ins = sponge_rows_of_blocks(groups)
    ends = np.flatnonzero(table[:, L.S_END] == 1)
    table[ends, L.D: L.D + 16] = sponge[sponge[:, SL.S_DIG] == 1, SL.V: SL.V + 16]
    words = table[table[:, L.R] == 1][:, [L.MSG, L.IDX, L.W_LO, L.W_HI]]
    msgs = np.concatenate([table[ends][:, [L.MSG, L.LEN]], table[ends, L.D: L.D + 16]], axis=1)
    return table, sponge, ins, words, msgs
