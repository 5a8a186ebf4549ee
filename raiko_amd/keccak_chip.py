"""The Keccak-f[1600] chip (rk_keccak_chip_air / rk_keccak_chip_trace, include/raiko_hip.h): the permutation behind
Keccak-256 as a table -- the first precompile-shaped chip, the shape of p3-keccak-air (pulled by the reference's
Cargo.lock, the crate itself outside the reference tree: RECALLED; the columns are this project's).  One row per round,
25 rows per permutation (row 24 is the output row: the permutation's output stands in the columns A its input stood in);
the AIR is written by the library, the rows on the GPU, one wavefront per permutation.

A state is 25 uint64 lanes, lane (x, y) at index x + 5 y; arrays of states are (n, 25) uint64.  The chip receives, per
permutation with multiplicity M, four tuples: (ID, limbs 0..49 of the input) on `bus`, (ID, limbs 50..99) on bus + 1,
and the two halves of the output on bus + 2, bus + 3 (limb index = 4 (x + 5 y) + limb, 16-bit limbs, little endian).
`claims_air` / `claims_rows` are the smallest table that uses it -- what an ecall table will look like --, and
`prove_permutations` proves [claims, chip] in one call.

Out of scope here: the chip as an ecall of the executor through the memory argument.  The sponge table for Keccak-256
of messages and the verifier-side claim form are raiko_amd/keccak_sponge.py."""
import ctypes as C

import numpy as np

from . import _lib, p3

BUS_KECCAK = 15              # .. 18; buses 1 .. 14 are taken
WAVES_PER_BLOCK = 4          # permutation slots per block of keccak_chip_trace_kernel (keccak_chip.hip)
ROWS_PER_PERMUTATION = 25


class Layout:
    """the chip's columns (kc::KeccakChipLayout, raiko_amd/csrc/keccak_chip.hpp)"""
    STEP = 0                 # [25] one-hot round flags
    A = 25                   # [25][4] the state entering the row, limbs
    C = 125                  # [5][64] column parities, bits
    CP = 445                 # [5][64] C' = C[x] ^ C[x-1] ^ rol(C[x+1], 1), bits
    AP = 765                 # [25][64] A': the state after theta, bits
    APP = 2365               # [25][4] A'': the state after rho, pi, chi, limbs
    APP00_BITS = 2465        # [64] the bits of A''[0][0]
    APPP00 = 2529            # [4] A'''[0][0]: lane (0, 0) after iota, limbs
    ID, M, M_IN, M_OUT = 2533, 2534, 2535, 2536
    WIDTH = 2537


def lanes_of(a):
    """raiko_amd.keccak's state a[x][y] -> 25 lanes, lane x + 5 y"""
    return np.array([a[i % 5][i // 5] for i in range(25)], dtype=np.uint64)


def limbs_of(states):
    """(n, 25) uint64 -> (n, 100) uint64: limb 4 i + l = bits 16 l .. 16 l + 15 of lane i"""
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 25)
    return np.stack([(s >> np.uint64(16 * l)) & np.uint64(0xFFFF) for l in range(4)], axis=2).reshape(-1, 100)


def min_rows(n):
    """the smallest table that holds n permutations: a power of two >= max(2, 25 n)"""
    return max(2, 1 << (ROWS_PER_PERMUTATION * int(n) - 1).bit_length())


def keccak_chip_air(params=None, bus=BUS_KECCAK):
    """rk_keccak_chip_air: the chip's AIR with its four receives (params None = the SP1 preset; it gives the extension's
    W).  The step list is written by the library; .steps is read back (rk_air_get_steps) so that a checker can evaluate
    it too; .layout names the columns."""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(None, lib.rk_keccak_chip_air(C.byref(params) if params is not None else None, bus, C.byref(h)))
    n = C.c_size_t(0)
    lib.rk_air_get_steps(h, None, 0, C.byref(n))
    steps = np.zeros((n.value, 3), dtype=np.uint32)
    _lib.check(None, lib.rk_air_get_steps(h, steps.ctypes.data, n.value, C.byref(n)))
    L = Layout
    halves = [list(range(L.A, L.A + 50)), list(range(L.A + 50, L.A + 100))]
    its = [p3.Interaction(p3.RECEIVE, bus + j, [L.ID] + halves[j & 1], L.M_IN if j < 2 else L.M_OUT) for j in range(4)]
    air = p3.Air(steps, int(lib.rk_keccak_chip_width()), 0, its)
    air._handle = h
    air.layout, air.bus = L, bus
    return air


def keccak_chip_trace(hal, states, ids=None, mult=None, rows=None):
    """rk_keccak_chip_trace: the chip's rows for `states` (n, 25) uint64 -> (device buffer rows x width row-major
    Montgomery words, ready as an on_device table; rows; the permutations' outputs (n, 25) uint64).  ids / mult: n
    Montgomery words each (None: 0 .. n - 1 / ones); rows: a power of two >= max(2, 25 n) (None: the smallest)"""
    from .hal import _ptr
    lib = _lib.load()
    s = np.ascontiguousarray(states, dtype=np.uint64).reshape(-1, 25)
    n = s.shape[0]
    rows = min_rows(n) if rows is None else int(rows)
    width = int(lib.rk_keccak_chip_width())
    if n == 0 or rows < 2 or rows & (rows - 1) or rows < ROWS_PER_PERMUTATION * n or rows > 1 << 24:
        raise _lib.RkError(_lib.RK_ERR_INVALID, "keccak_chip_trace: n = %d permutations do not fit rows = %d" % (n, rows))
    d_in = hal.copy_from_elem(s.view(np.uint32).reshape(-1))
    d_ids = hal.copy_from_elem(np.ascontiguousarray(ids, dtype=np.uint32)) if ids is not None else None
    d_mult = hal.copy_from_elem(np.ascontiguousarray(mult, dtype=np.uint32)) if mult is not None else None
    assert (d_ids is None or d_ids.size() == n) and (d_mult is None or d_mult.size() == n)
    d_rows = hal.alloc_elem(rows * width)
    d_out = hal.alloc_elem(n * 50)
    _lib.check(hal._ctx, lib.rk_keccak_chip_trace(hal._ctx, _ptr(d_in), _ptr(d_ids) if d_ids is not None else None,
                                                  _ptr(d_mult) if d_mult is not None else None, n, rows, _ptr(d_rows), _ptr(d_out)))
    return d_rows, rows, d_out.to_host().view(np.uint64).reshape(n, 25)


def keccak_chip_table(hal, states, ids=None, mult=None, rows=None, air=None):
    """the chip's table with its rows in HBM: a Table without a host trace, its height pinned; .device = (DeviceBuffer,
    log_height), what p3.prove's device_traces takes; .outputs = the permutations' outputs"""
    d_rows, rows, outs = keccak_chip_trace(hal, states, ids, mult, rows)
    t = p3.Table.pinned(air if air is not None else keccak_chip_air(), rows.bit_length() - 1)
    t.device, t.outputs = (d_rows, rows.bit_length() - 1), outs
    return t


def claims_air(ext_w=p3.EXT_W, bus=BUS_KECCAK):
    """the smallest table that uses the chip: ID | V[50] | S0 .. S3 (55 columns).  A row with S_j = 1 sends (ID, V) on
    bus + j: half a state, the input's (j = 0, 1) or the output's (j = 2, 3).  Every S_j and their sum are boolean."""
    b = p3.AirBuilder(55, 0, ext_w)
    s = [b.local(51 + j) for j in range(4)]
    for v in s:
        b.assert_zero(v * (v - 1))
    total = s[0] + s[1] + s[2] + s[3]
    b.assert_zero(total * (total - 1))
    for j in range(4):
        b.send(bus + j, list(range(51)), mult=51 + j, mult_is_const=False)
    return b.build(library_constraints=True)


def claims_rows(states_in, states_out, ids=None):
    """rows of claims_air (canonical uint64): four per permutation -- the two halves of its input, the two of its output
    --, padded with zero rows to a power of two.  ids: canonical (None: 0 .. n - 1)"""
    lin, lout = limbs_of(states_in), limbs_of(states_out)
    n = lin.shape[0]
    ids = np.arange(n, dtype=np.uint64) if ids is None else np.asarray(ids, dtype=np.uint64)
    out = np.zeros((max(2, 1 << (4 * n - 1).bit_length()), 55), dtype=np.uint64)
    for j in range(4):
        src = lin if j < 2 else lout
        out[j: 4 * n: 4, 0] = ids
        out[j: 4 * n: 4, 1:51] = src[:, 50 * (j & 1): 50 * (j & 1) + 50]
        out[j: 4 * n: 4, 51 + j] = 1
    return out


def prove_permutations(hal, states, params=None):
    """Keccak-f[1600] of `states` (n, 25) uint64, proven: the chip's rows on the GPU, a claims table sending every (input,
    output) pair, rk_p3_prove over [claims, chip] under hal's parameter set (params: its blob, for an extension other
    than the SP1 preset's) -> (proof words, outputs (n, 25) uint64, [claims table, chip table]); p3.verify takes the
    tables as they are"""
    from .hal import _ptr
    ext_w = int(params.ext_w) if params is not None else p3.EXT_W
    chip = keccak_chip_table(hal, states, air=keccak_chip_air(params))
    claims = p3.Table.from_canonical(claims_air(ext_w), claims_rows(states, chip.outputs))
    tables = [claims, chip]
    proof = p3.prove(hal, tables, device_traces=[None, (_ptr(chip.device[0]), chip.device[1])])
    return proof, chip.outputs, tables
