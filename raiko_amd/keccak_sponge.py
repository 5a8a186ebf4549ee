"""The Keccak-256 sponge table (rk_keccak_sponge_air / rk_keccak_sponge_trace, include/raiko_hip.h) over the
Keccak-f[1600] chip (raiko_amd/keccak_chip.py): "the Keccak-256 of these bytes is this digest", proven over two tables
[sponge, chip].  Rate 136 bytes, padding 0x01 .. 0x80 as raiko_amd.keccak.keccak256 (not SHA-3's 0x06), output the first
four lanes.  The table absorbs whole blocks: padding lies with whoever sends them -- here the verifier, which pads its own
messages when it forms the claims (`statement`), later an ecall table.  The AIR has no padding constraints.

Three rows per block (the block X, the permutation's input I, its output O); everything sent stands in the one block V
of 100 limb columns.  Sends: (PID, half of V) to the chip on bus .. bus + 3, the block as (MSG, BLK, 34 limbs) on
bus + 4, bus + 5 and (MSG, NBLK, 16 digest limbs) on bus + 6.  No table receives the last three: the verifier does,
through p3.verify(claims=).

What the claim form costs and what it does not give: `statement` puts every claim tuple into the init words, which the
transcript observes before any challenge exists -- the binding rk_p3_verify_claims demands --, so the verifier's work
is LINEAR in the messages (it pads them, observes 72 words a block and inverts one extension element a tuple) and this
form does not spare the verifier the bytes.  It is the harness that makes the table testable end to end with public
messages, and its sends are the interface an ecall table will receive.

The padding in circuit, for a sender that knows words and a byte length only, is the table under this one:
raiko_amd/keccak_pad.py.

Out of scope: the executor's ecall (RK_ECALL_KECCAK), SHA-3 padding and other rates, a Poseidon2-digest binding of the
claims in place of init."""
import ctypes as C

import numpy as np

from . import _lib, keccak_chip, p3

RATE = 136                   # bytes a block = 17 lanes = 68 limbs
ROWS_PER_BLOCK = 3
WAVES_PER_BLOCK = 4          # block slots per thread block of keccak_sponge_rows_kernel (keccak_sponge.hip)
CHAIN_WAVES_PER_BLOCK = 4    # messages per thread block of keccak_sponge_chain_kernel


class Layout:
    """the sponge's columns (kc::KeccakSpongeLayout, raiko_amd/csrc/keccak_sponge.hpp)"""
    V = 0                    # [100] the block (X row: 68 limbs, then 0), the permutation's input (I), its output (O)
    PREV = 100               # [100] the state before this block, the same on a group's three rows
    MB = 200                 # [17][64] the bits of V's rate lanes
    PB = 1288                # [17][64] the bits of PREV's rate lanes
    XR = 2376                # [68] sum_k 2^k (mb ^ pb)
    MSG, BLK, NBLK, PID = 2444, 2445, 2446, 2447
    KX, KI, KO, REAL = 2448, 2449, 2450, 2451
    FIRST, LAST = 2452, 2453
    S_IN, S_OUT, S_MSG, S_DIG = 2454, 2455, 2456, 2457
    WIDTH = 2458


def pad_blocks(messages):
    """byte strings -> (blocks (n_blocks, 17) uint64, first (k + 1,) uint32: the first block of each message, then
    n_blocks).  Keccak-256's padding: 0x01, zeros, 0x80 into the last byte of a 136-byte block (0x81 where they meet)"""
    out, first = [], [0]
    for m in messages:
        b = bytearray(bytes(m))
        b.append(0x01)
        b += bytes(-len(b) % RATE)
        b[-1] |= 0x80
        out.append(np.frombuffer(bytes(b), dtype="<u8").reshape(-1, 17))
        first.append(first[-1] + out[-1].shape[0])
    blocks = np.concatenate(out).astype(np.uint64) if out else np.zeros((0, 17), dtype=np.uint64)
    return np.ascontiguousarray(blocks), np.array(first, dtype=np.uint32)


def min_rows(n_blocks):
    """the smallest table that holds n_blocks blocks: a power of two >= max(2, 3 n_blocks)"""
    return max(2, 1 << (ROWS_PER_BLOCK * int(n_blocks) - 1).bit_length())


def keccak_sponge_air(params=None, bus=keccak_chip.BUS_KECCAK):
    """rk_keccak_sponge_air: the sponge's AIR with its seven sends (params None = the SP1 preset; it gives the
    extension's W).  The step list is written by the library; .steps is read back (rk_air_get_steps) so that a checker
    can evaluate it too; .layout names the columns."""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(None, lib.rk_keccak_sponge_air(C.byref(params) if params is not None else None, bus, C.byref(h)))
    n = C.c_size_t(0)
    lib.rk_air_get_steps(h, None, 0, C.byref(n))
    steps = np.zeros((n.value, 3), dtype=np.uint32)
    _lib.check(None, lib.rk_air_get_steps(h, steps.ctypes.data, n.value, C.byref(n)))
    L = Layout
    v = lambda lo, hi: list(range(L.V + lo, L.V + hi))
    its = [p3.Interaction(p3.SEND, bus + j, [L.PID] + v(50 * (j & 1), 50 * (j & 1) + 50), L.S_IN if j < 2 else L.S_OUT) for j in range(4)]
    its += [p3.Interaction(p3.SEND, bus + 4 + j, [L.MSG, L.BLK] + v(34 * j, 34 * j + 34), L.S_MSG) for j in range(2)]
    its.append(p3.Interaction(p3.SEND, bus + 6, [L.MSG, L.NBLK] + v(0, 16), L.S_DIG))
    air = p3.Air(steps, int(lib.rk_keccak_sponge_width()), 0, its)
    air._handle = h
    air.layout, air.bus = L, bus
    return air


class SpongeTrace:
    """what rk_keccak_sponge_trace left: .d_rows (device, rows x width Montgomery words), .rows, .d_states (device,
    n_blocks x 25 lanes: what rk_keccak_chip_trace reads), .d_digests (device, k x 4 lanes), .n_blocks, and on the host .states / .outs (n_blocks, 25)
    uint64, .digests (k, 4) uint64"""


def keccak_sponge_trace(hal, messages, msg_ids=None, rows=None):
    """rk_keccak_sponge_trace for byte strings `messages` (padded here) -> SpongeTrace.  msg_ids: one Montgomery word
    a message (None: 0 .. k - 1); rows: a power of two >= max(2, 3 n_blocks) (None: the smallest)"""
    blocks, first = pad_blocks(messages)
    k, nb = len(first) - 1, blocks.shape[0]
    rows = min_rows(nb) if rows is None else int(rows)
    if k == 0 or rows < 2 or rows & (rows - 1) or rows < ROWS_PER_BLOCK * nb or rows > 1 << 24:
        raise _lib.RkError(_lib.RK_ERR_INVALID, "keccak_sponge_trace: %d messages, %d blocks do not fit rows = %d" % (k, nb, rows))
    d_blocks = hal.copy_from_elem(blocks.view(np.uint32).reshape(-1))
    d_first = hal.copy_from_elem(first)
    d_ids = hal.copy_from_elem(np.ascontiguousarray(msg_ids, dtype=np.uint32)) if msg_ids is not None else None
    assert d_ids is None or d_ids.size() == k
    return keccak_sponge_trace_device(hal, d_blocks, d_first, d_ids, k, nb, rows)


def keccak_sponge_trace_device(hal, d_blocks, d_first, d_ids, k, nb, rows):
    """rk_keccak_sponge_trace over blocks that are in HBM already -> SpongeTrace (with .d_digests, the k x 4 lanes on the
    device).  d_blocks nb x 17 lanes, d_first k + 1 words, d_ids k Montgomery words or None: DeviceBuffers"""
    from .hal import _ptr
    lib = _lib.load()
    width = int(lib.rk_keccak_sponge_width())
    t = SpongeTrace()
    t.rows, t.n_blocks = rows, nb
    t.d_rows, t.d_states = hal.alloc_elem(rows * width), hal.alloc_elem(nb * 50)
    d_outs, t.d_digests = hal.alloc_elem(nb * 50), hal.alloc_elem(k * 8)
    _lib.check(hal._ctx, lib.rk_keccak_sponge_trace(hal._ctx, _ptr(d_blocks), _ptr(d_first), _ptr(d_ids) if d_ids is not None else None, k, nb,
                                                    rows, _ptr(t.d_rows), _ptr(t.d_states), _ptr(d_outs), _ptr(t.d_digests)))
    t.states = t.d_states.to_host().view(np.uint64).reshape(nb, 25)
    t.outs = d_outs.to_host().view(np.uint64).reshape(nb, 25)
    t.digests = t.d_digests.to_host().view(np.uint64).reshape(k, 4)
    return t


def keccak_sponge_tables(hal, messages, params=None):
    """[sponge table, chip table] with their rows in HBM (Tables without a host trace, heights pinned, .device =
    (DeviceBuffer, log_height)): the sponge's by rk_keccak_sponge_trace, the chip's by rk_keccak_chip_trace straight
    from the d_states buffer the chain kernel left on the device.  The sponge table carries .trace_info (SpongeTrace)"""
    return tables_of_trace(hal, keccak_sponge_trace(hal, messages), params)


def tables_of_trace(hal, t, params=None):
    """[sponge table, chip table] of a SpongeTrace, as keccak_sponge_tables describes them"""
    from .hal import _ptr
    lib = _lib.load()
    sponge = p3.Table.pinned(keccak_sponge_air(params), t.rows.bit_length() - 1)
    sponge.device, sponge.trace_info = (t.d_rows, t.rows.bit_length() - 1), t
    chip_rows = keccak_chip.min_rows(t.n_blocks)
    d_chip = hal.alloc_elem(chip_rows * int(lib.rk_keccak_chip_width()))
    _lib.check(hal._ctx, lib.rk_keccak_chip_trace(hal._ctx, _ptr(t.d_states), None, None, t.n_blocks, chip_rows, _ptr(d_chip), None))
    chip = p3.Table.pinned(keccak_chip.keccak_chip_air(params), chip_rows.bit_length() - 1)
    chip.device = (d_chip, chip_rows.bit_length() - 1)
    return [sponge, chip]


def digest_bytes(digests):
    """(k, 4) uint64 -> k 32-byte strings"""
    return [np.ascontiguousarray(d, dtype="<u8").tobytes() for d in np.asarray(digests, dtype=np.uint64).reshape(-1, 4)]


def statement(messages, digests, bus=keccak_chip.BUS_KECCAK):
    """what the verifier forms from ITS messages and digests (32-byte strings) -> (init words, claims).  claims =
    [(bus + 4, -1, tuples), (bus + 5, -1, tuples), (bus + 6, -1, tuples)] in Montgomery words, as p3.verify(claims=)
    takes them: per block (message number, block number, limbs 0..33 / 34..67 of the padded block), per message
    (message number, block count, the digest's 16 limbs).  init = Montgomery words of [k, the block count of every
    message, every claim tuple's canonical words in claim order]: observed before the challenges exist, which is the
    binding rk_p3_verify_claims leaves to its caller.  The cost: linear in the messages -- this form does not spare the
    verifier the bytes (see the module's docstring)"""
    messages, digests = list(messages), list(digests)
    if len(messages) != len(digests) or not messages or any(len(d) != 32 for d in digests):
        raise ValueError("statement: one 32-byte digest a message, at least one message")
    blocks, first = pad_blocks(messages)
    counts = np.diff(first.astype(np.int64))
    limbs = keccak_chip.limbs_of(np.concatenate([blocks, np.zeros((blocks.shape[0], 8), dtype=np.uint64)], axis=1))[:, :68]
    msg = np.repeat(np.arange(len(messages), dtype=np.uint64), counts)
    blk = np.concatenate([np.arange(c, dtype=np.uint64) for c in counts])
    halves = [np.concatenate([msg[:, None], blk[:, None], limbs[:, 34 * j: 34 * j + 34]], axis=1) for j in range(2)]
    dig = np.frombuffer(b"".join(digests), dtype="<u2").reshape(-1, 16).astype(np.uint64)
    ends = np.concatenate([np.arange(len(messages), dtype=np.uint64)[:, None], counts.astype(np.uint64)[:, None], dig], axis=1)
    tuples = halves + [ends]
    init = np.concatenate([np.array([len(messages)], dtype=np.uint64), counts.astype(np.uint64)] + [t.reshape(-1) for t in tuples])
    return p3.to_mont(init), [(bus + 4 + j, -1, p3.to_mont(t)) for j, t in enumerate(tuples)]


def prove_keccak256(hal, messages, params=None):
    """Keccak-256 of `messages`, proven: both tables' rows written on the GPU, rk_p3_prove over [sponge, chip] under
    hal's parameter set (params: its blob, for an extension other than the SP1 preset's) with `statement`'s init words
    -> (proof words, digests: 32-byte strings, [sponge table, chip table])"""
    from .hal import _ptr
    tables = keccak_sponge_tables(hal, messages, params)
    digests = digest_bytes(tables[0].trace_info.digests)
    init, _claims = statement(messages, digests)
    proof = p3.prove(hal, tables, init, device_traces=[(_ptr(t.device[0]), t.device[1]) for t in tables])
    return proof, digests, tables


def verify_keccak256(messages, digests, proof, params=None) -> int:
    """0 exactly when `proof` shows digests[i] = Keccak-256(messages[i]) for every i (else rk_p3_verify's reason).  Host
    only, and handed nothing by the prover but the proof: both AIRs are built here, both heights pinned from the block
    counts alone, init words and receive claims formed from the verifier's own messages and digests"""
    init, claims = statement(messages, digests)
    nb = sum(len(bytes(m)) // RATE + 1 for m in messages)
    tables = [p3.Table.pinned(keccak_sponge_air(params), min_rows(nb).bit_length() - 1),
              p3.Table.pinned(keccak_chip.keccak_chip_air(params), keccak_chip.min_rows(nb).bit_length() - 1)]
    return p3.verify(tables, proof, init, params=params, claims=claims)
