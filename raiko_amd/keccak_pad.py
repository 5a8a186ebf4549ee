"""The Keccak-256 padding table (rk_keccak_pad_air / rk_keccak_pad_trace, include/raiko_hip.h) under the sponge table
(raiko_amd/keccak_sponge.py): "the Keccak-256 of the first len bytes of these 32-bit words is this digest", proven over
three tables [pad, sponge, chip].  The sender of a message knows its little-endian words, NW = ceil(len / 4) of them,
and its byte length -- what a row of a memory-argument table can hand over -- and nothing about 0x01 .. 0x80; the bytes
of the last word past len are arbitrary and do not reach the hash.

One row per word slot, 34 rows per 136-byte block.  The table receives the sponge's three sends (the block's two halves
on bus + 4, bus + 5, block count and digest on bus + 6) and sends (MSG, IDX, W_LO, W_HI) on bus + 7, one a word, and
(MSG, LEN, 16 digest limbs) on bus + 8, one a message.  No table receives those two: the verifier does, through
p3.verify(claims=) with `statement_words`, and it never pads.  Padding is done on the device: the blocks kernel writes
the padded blocks the sponge's kernels read, the rows kernel this table's rows, and once the sponge has run,
rk_keccak_pad_digests puts the digests into D.

Out of scope: RK_ECALL_KECCAK itself (the executor's ecall, io-table rows that send the words, the digest's write-back,
key and shard pool), sources that are not word-aligned, SHA-3's 0x06."""
import ctypes as C

import numpy as np

from . import _lib, keccak_chip, keccak_sponge, p3

ROWS_PER_BLOCK = 34
ROWS_WAVES_PER_BLOCK = 4     # block slots per thread block of keccak_pad_rows_kernel (keccak_pad.hip)
BLOCKS_THREADS = 256         # word slots per thread block of keccak_pad_blocks_kernel: 7 blocks fit one, the 8th starts a second


class Layout:
    """the table's columns (kc::KeccakPadLayout, raiko_amd/csrc/keccak_pad.hpp)"""
    B = 0                    # [68] the shift register of limbs: B[66], B[67] the word placed on this row
    STEP = 68                # [34] one-hot word position in the block
    W_LO, W_HI = 102, 103    # the sender's word
    WB = 104                 # [32] its bits
    E = 136                  # [4] one-hot of len mod 4 on the END row
    D = 140                  # [16] the digest's limbs on a message's last row
    MSG, BLK, NBLK, IDX, LEN = 156, 157, 158, 159, 160
    DATA, END, AFTER, REAL = 161, 162, 163, 164
    R, S_END = 165, 166
    WIDTH = 167


def n_blocks_of(length):
    return int(length) // keccak_sponge.RATE + 1


def words_of(messages, tail=None):
    """byte strings -> (words uint32: the messages' little-endian words back to back, ceil(len / 4) each; word_first
    (k + 1,) uint32; lens (k,) uint32; first (k + 1,) uint32: the first block of each message, then n_blocks).  tail:
    per message the bytes that stand past its end in its last word (None: zeros)"""
    words, word_first, lens, first = [], [0], [], [0]
    for i, m in enumerate(messages):
        m = bytes(m)
        fill = (bytes(tail[i]) if tail is not None else b"") + bytes(3)
        words.append(np.frombuffer(m + fill[: -len(m) % 4], dtype="<u4"))
        word_first.append(word_first[-1] + words[-1].size)
        lens.append(len(m))
        first.append(first[-1] + n_blocks_of(len(m)))
    words = np.concatenate(words).astype(np.uint32) if words else np.zeros(0, dtype=np.uint32)
    return np.ascontiguousarray(words), np.array(word_first, dtype=np.uint32), np.array(lens, dtype=np.uint32), np.array(first, dtype=np.uint32)


def min_rows(n_blocks):
    """the smallest table that holds n_blocks blocks: a power of two >= 34 n_blocks"""
    return 1 << (ROWS_PER_BLOCK * int(n_blocks) - 1).bit_length()


def keccak_pad_air(params=None, bus=keccak_chip.BUS_KECCAK):
    """rk_keccak_pad_air: the table's AIR with its three receives and two sends (params None = the SP1 preset).  The step
    list is written by the library; .steps is read back so that a checker can evaluate it too; .layout names the columns."""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(None, lib.rk_keccak_pad_air(C.byref(params) if params is not None else None, bus, C.byref(h)))
    n = C.c_size_t(0)
    lib.rk_air_get_steps(h, None, 0, C.byref(n))
    steps = np.zeros((n.value, 3), dtype=np.uint32)
    _lib.check(None, lib.rk_air_get_steps(h, steps.ctypes.data, n.value, C.byref(n)))
    L = Layout
    b, d = (lambda lo, hi: list(range(L.B + lo, L.B + hi))), list(range(L.D, L.D + 16))
    its = [p3.Interaction(p3.RECEIVE, bus + 4 + j, [L.MSG, L.BLK] + b(34 * j, 34 * j + 34), L.STEP + 33) for j in range(2)]
    its.append(p3.Interaction(p3.RECEIVE, bus + 6, [L.MSG, L.NBLK] + d, L.S_END))
    its.append(p3.Interaction(p3.SEND, bus + 7, [L.MSG, L.IDX, L.W_LO, L.W_HI], L.R))
    its.append(p3.Interaction(p3.SEND, bus + 8, [L.MSG, L.LEN] + d, L.S_END))
    air = p3.Air(steps, int(lib.rk_keccak_pad_width()), 0, its)
    air._handle = h
    air.layout, air.bus = L, bus
    return air


class PadTrace:
    """what rk_keccak_pad_trace left: .d_rows (device, rows x width Montgomery words, D = 0 until put_digests), .rows,
    .d_blocks (device, n_blocks x 17 lanes: what rk_keccak_sponge_trace reads), .d_first, .d_ids, .d_inputs (the words, their firsts and the lengths: kept while the launches may run), .n_msgs,
    .n_blocks"""

    def blocks(self):
        """the padded blocks, read back: (n_blocks, 17) uint64"""
        return self.d_blocks.to_host().view(np.uint64).reshape(self.n_blocks, 17)


def keccak_pad_trace(hal, messages, msg_ids=None, rows=None, tail=None):
    """rk_keccak_pad_trace for byte strings `messages` -> PadTrace.  msg_ids: one Montgomery word a message (None:
    0 .. k - 1); rows: a power of two >= 34 n_blocks (None: the smallest); tail: as words_of"""
    from .hal import _ptr
    lib = _lib.load()
    words, word_first, lens, first = words_of(messages, tail)
    k, nb = len(lens), int(first[-1])
    rows = min_rows(nb) if rows is None else int(rows)
    if k == 0 or rows & (rows - 1) or rows < ROWS_PER_BLOCK * nb or rows > 1 << 24:
        raise _lib.RkError(_lib.RK_ERR_INVALID, "keccak_pad_trace: %d messages, %d blocks do not fit rows = %d" % (k, nb, rows))
    t = PadTrace()
    t.d_inputs = d_words, d_word_first, d_lens = [hal.copy_from_elem(a) for a in (words if words.size else np.zeros(1, dtype=np.uint32), word_first, lens)]
    t.rows, t.n_msgs, t.n_blocks = rows, k, nb
    t.d_first = hal.copy_from_elem(first)
    t.d_ids = hal.copy_from_elem(np.ascontiguousarray(msg_ids, dtype=np.uint32)) if msg_ids is not None else None
    assert t.d_ids is None or t.d_ids.size() == k
    t.d_rows, t.d_blocks = hal.alloc_elem(rows * Layout.WIDTH), hal.alloc_elem(nb * 34)
    _lib.check(hal._ctx, lib.rk_keccak_pad_trace(hal._ctx, _ptr(d_words), words.size, _ptr(d_word_first), _ptr(d_lens), _ptr(t.d_first),
                                                 _ptr(t.d_ids) if t.d_ids is not None else None, k, nb, rows, _ptr(t.d_rows), _ptr(t.d_blocks)))
    return t


def put_digests(hal, t, d_digests):
    """rk_keccak_pad_digests: D of every message's last row from the sponge's d_digests (device, k x 4 lanes)"""
    from .hal import _ptr
    lib = _lib.load()
    _lib.check(hal._ctx, lib.rk_keccak_pad_digests(hal._ctx, _ptr(d_digests), _ptr(t.d_first), t.n_msgs, t.n_blocks, t.rows, _ptr(t.d_rows)))


def keccak_pad_tables(hal, messages, params=None, tail=None):
    """[pad table, sponge table, chip table] with their rows in HBM (heights pinned, .device = (DeviceBuffer,
    log_height)).  The sponge's d_blocks are the pad kernel's output, left on the device: the padded message is never
    formed on the host.  The pad table carries .trace_info (PadTrace), the sponge table its SpongeTrace"""
    t = keccak_pad_trace(hal, messages, tail=tail)
    st = keccak_sponge.keccak_sponge_trace_device(hal, t.d_blocks, t.d_first, None, t.n_msgs, t.n_blocks, keccak_sponge.min_rows(t.n_blocks))
    put_digests(hal, t, st.d_digests)
    pad = p3.Table.pinned(keccak_pad_air(params), t.rows.bit_length() - 1)
    pad.device, pad.trace_info = (t.d_rows, t.rows.bit_length() - 1), t
    return [pad] + keccak_sponge.tables_of_trace(hal, st, params)


def statement_words(messages, digests, bus=keccak_chip.BUS_KECCAK, tail=None):
    """what the verifier forms from ITS messages and digests (32-byte strings) -> (init words, claims).  claims =
    [(bus + 7, -1, tuples), (bus + 8, -1, tuples)] in Montgomery words, as p3.verify(claims=) takes them: per word
    (message number, word index, low limb, high limb), per message (message number, byte length, the digest's 16
    limbs).  init = Montgomery words of [k, every len, every claim tuple's canonical words in claim order]: observed
    before the challenges exist, the binding rk_p3_verify_claims leaves to its caller.  Nothing is padded here"""
    messages, digests = [bytes(m) for m in messages], list(digests)
    if len(messages) != len(digests) or not messages or any(len(d) != 32 for d in digests):
        raise ValueError("statement_words: one 32-byte digest a message, at least one message")
    words, word_first, lens, _first = words_of(messages, tail)
    counts = np.diff(word_first.astype(np.int64))
    msg = np.repeat(np.arange(len(messages), dtype=np.uint64), counts)
    idx = np.concatenate([np.arange(c, dtype=np.uint64) for c in counts])
    w = words.astype(np.uint64)
    per_word = np.stack([msg, idx, w & np.uint64(0xFFFF), w >> np.uint64(16)], axis=1).reshape(-1, 4)
    dig = np.frombuffer(b"".join(digests), dtype="<u2").reshape(-1, 16).astype(np.uint64)
    per_msg = np.concatenate([np.arange(len(messages), dtype=np.uint64)[:, None], lens.astype(np.uint64)[:, None], dig], axis=1)
    tuples = [per_word, per_msg]
    init = np.concatenate([np.array([len(messages)], dtype=np.uint64), lens.astype(np.uint64)] + [t.reshape(-1) for t in tuples])
    return p3.to_mont(init), [(bus + 7 + j, -1, p3.to_mont(t)) for j, t in enumerate(tuples)]


def prove_keccak256_words(hal, messages, params=None, tail=None):
    """Keccak-256 of `messages`, proven from their words: the three tables' rows written on the GPU, rk_p3_prove over
    [pad, sponge, chip] with `statement_words`' init words -> (proof words, digests: 32-byte strings, the tables)"""
    from .hal import _ptr
    tables = keccak_pad_tables(hal, messages, params, tail)
    digests = keccak_sponge.digest_bytes(tables[1].trace_info.digests)
    init, _claims = statement_words(messages, digests, tail=tail)
    proof = p3.prove(hal, tables, init, device_traces=[(_ptr(t.device[0]), t.device[1]) for t in tables])
    return proof, digests, tables


def verify_keccak256_words(messages, digests, proof, params=None, tail=None) -> int:
    """0 exactly when `proof` shows digests[i] = Keccak-256(messages[i]) for every i (else rk_p3_verify's reason).  Host
    only, and handed nothing by the prover but the proof: the three AIRs are built here, all heights pinned from the
    lengths alone, init words and receive claims formed from the verifier's own words, lengths and digests"""
    init, claims = statement_words(messages, digests, tail=tail)
    nb = sum(n_blocks_of(len(bytes(m))) for m in messages)
    tables = [p3.Table.pinned(keccak_pad_air(params), min_rows(nb).bit_length() - 1),
              p3.Table.pinned(keccak_sponge.keccak_sponge_air(params), keccak_sponge.min_rows(nb).bit_length() - 1),
              p3.Table.pinned(keccak_chip.keccak_chip_air(params), keccak_chip.min_rows(nb).bit_length() - 1)]
    return p3.verify(tables, proof, init, params=params, claims=claims)
