"""The Keccak-f[1600] chip on the GPU (rk_keccak_chip_trace, keccak_chip.hip; raiko_amd/keccak_chip.py): the rows the
kernel writes equal the numpy restatement (tests/keccak_chip_ref.py) word for word at every launch threshold -- one slot,
the slot the table's end cuts off, one full block, the first second block, a table half of whose slots are padding --,
the outputs it reports are Keccak-f[1600], a proof over the device rows equals the oracle's over the restatement's, and
the refusals leave the context usable."""
import ctypes as C

import numpy as np
import pytest

import keccak_chip_ref as R
import oracle_lib as o
from raiko_amd import _lib, hal, keccak, keccak_chip as K, p3

pytestmark = pytest.mark.gpu

P = o.P
W = K.WAVES_PER_BLOCK
# n = 1 (32 rows), 2, 5 (the cut-off slot), W (one full block), W + 1 (the first second block), 41 (1025 rows: a 2048-row
# table of which about half is padding slots), and one permutation in 64 rows (whole padding permutations)
SHAPES = sorted({(1, 32), (2, 64), (5, 128), (W, K.min_rows(W)), (W + 1, K.min_rows(W + 1)), (41, 2048), (1, 64)})


@pytest.fixture(scope="module")
def gpu():
    h = hal.HipHal(0)
    yield h
    h.close()


def f1600(lanes):
    a = [[int(lanes[x + 5 * y]) for y in range(5)] for x in range(5)]
    return K.lanes_of(keccak._f1600(a))


@pytest.mark.parametrize("n,rows", SHAPES)
def test_gpu_rows_equal_the_restatement(gpu, n, rows):
    rng = np.random.default_rng(100 + n + rows)
    states = rng.integers(0, 1 << 64, size=(n, 25), dtype=np.uint64)
    d_rows, got_rows, outs = K.keccak_chip_trace(gpu, states, rows=rows)
    assert got_rows == rows and (rows == K.min_rows(n) or (n, rows) == (1, 64))
    assert np.array_equal(d_rows.to_host().reshape(rows, K.Layout.WIDTH), p3.to_mont(R.chip_rows(states, rows=rows)))
    want_out = np.stack([f1600(s) for s in states])
    assert np.array_equal(outs, want_out)
    ids, mult = rng.integers(0, P, size=n), rng.choice([0, 1, 3], size=n)
    d_rows, _, outs = K.keccak_chip_trace(gpu, states, p3.to_mont(ids), p3.to_mont(mult), rows)
    assert np.array_equal(d_rows.to_host().reshape(rows, K.Layout.WIDTH), p3.to_mont(R.chip_rows(states, ids, mult, rows)))
    assert np.array_equal(outs, want_out)


@pytest.mark.parametrize("n", [1, 5])
def test_gpu_proof_over_device_rows_is_the_oracles(gpu, n):
    over = dict(queries=4, pow_bits=2)
    try:
        blob = gpu.set_params(1, **over)
        o.oracle_set_params(1, **over)
        states = np.random.default_rng(200 + n).integers(0, 1 << 64, size=(n, 25), dtype=np.uint64)
        proof, outs, tables = K.prove_permutations(gpu, states, params=blob)
        assert np.array_equal(outs, np.stack([f1600(s) for s in states]))
        host = [tables[0], p3.Table.from_canonical(tables[1].air, R.chip_rows(states))]
        assert np.array_equal(proof, o.oracle_p3_prove(host))          # the oracle proves the numpy rows: this holds the device rows too
        assert p3.verify(tables, proof, params=blob) == 0 == p3.verify(host, proof, params=blob)
    finally:
        o.oracle_set_params()
        gpu.set_params(1)


def test_gpu_refusals_leave_the_context_usable(gpu):
    lib = _lib.load()
    states = np.random.default_rng(3).integers(0, 1 << 64, size=(2, 25), dtype=np.uint64)
    d_in = gpu.copy_from_elem(states.view(np.uint32).reshape(-1))
    d_rows = gpu.alloc_elem(64 * K.Layout.WIDTH)
    call = lambda ctx, s, t, n, rows: lib.rk_keccak_chip_trace(ctx, s, None, None, n, rows, t, None)
    ctx, s, t = gpu._ctx, d_in.ptr, d_rows.ptr
    assert call(None, s, t, 2, 64) == _lib.RK_ERR_INVALID
    assert call(ctx, None, t, 2, 64) == _lib.RK_ERR_INVALID
    assert call(ctx, s, None, 2, 64) == _lib.RK_ERR_INVALID
    assert call(ctx, s, t, 0, 64) == _lib.RK_ERR_INVALID
    assert call(ctx, s, t, 2, 48) == _lib.RK_ERR_INVALID              # no power of two
    assert call(ctx, s, t, 2, 32) == _lib.RK_ERR_INVALID              # below 25 n
    assert call(ctx, s, t, 1, 1) == _lib.RK_ERR_INVALID
    assert call(ctx, s, t, 2, 1 << 25) == _lib.RK_ERR_INVALID         # above 2^24
    assert call(ctx, s, t, 2, 64) == 0
    assert np.array_equal(d_rows.to_host().reshape(64, K.Layout.WIDTH), p3.to_mont(R.chip_rows(states)))
