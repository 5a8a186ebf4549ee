"""The Keccak-256 sponge table on the GPU (rk_keccak_sponge_trace, keccak_sponge.hip; raiko_amd/keccak_sponge.py): the
rows the two kernels write equal the numpy restatement (tests/keccak_sponge_ref.py) word for word at every launch
threshold -- one block, the pad byte 0x81, a block of padding alone, a full thread block and the first second one of
either kernel, a nine-block chain, a table half of whose slots are padding, given message IDs --, the states, outputs
and digests they report are Keccak-f[1600] chained by hand and Keccak-256, the chip's rows written from the states
buffer on the device are the chip's restatement, a proof over the device tables equals the oracle's over the
restatement's, verify_keccak256 accepts it and refuses a flipped message bit, and the refusals leave the context usable."""
import numpy as np
import pytest

import keccak_chip_ref as CR
import keccak_sponge_ref as R
import oracle_lib as o
from raiko_amd import _lib, hal, keccak, keccak_chip as K, keccak_sponge as S, p3

pytestmark = pytest.mark.gpu

L = S.Layout
CASES = R.kernel_cases(S.WAVES_PER_BLOCK, S.CHAIN_WAVES_PER_BLOCK)


@pytest.fixture(scope="module")
def gpu():
    h = hal.HipHal(0)
    yield h
    h.close()


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_rows_equal_the_restatement(gpu, name):
    msgs, ids, rows = CASES[name]
    t = S.keccak_sponge_trace(gpu, msgs, None if ids is None else p3.to_mont(ids), rows)
    chains = [R.chain(m) for m in msgs]
    n_blocks = sum(c[0].shape[0] for c in chains)
    assert t.n_blocks == n_blocks and t.rows == (S.min_rows(n_blocks) if rows is None else rows)
    assert np.array_equal(t.d_rows.to_host().reshape(t.rows, L.WIDTH), p3.to_mont(R.sponge_rows(msgs, ids, rows)))
    assert np.array_equal(t.states, np.concatenate([c[1] for c in chains])) and np.array_equal(t.outs, np.concatenate([c[2] for c in chains]))
    assert S.digest_bytes(t.digests) == [keccak.keccak256(m) for m in msgs]


def test_gpu_chip_rows_from_the_states_on_the_device(gpu):
    msgs = R.set_12131()
    sponge, chip = S.keccak_sponge_tables(gpu, msgs)
    t = sponge.trace_info
    assert chip.device[1] == 8 and sponge.device[1] == 5 and t.n_blocks == 8
    assert np.array_equal(chip.device[0].to_host().reshape(256, K.Layout.WIDTH), p3.to_mont(CR.chip_rows(t.states)))
    assert np.array_equal(t.states, np.concatenate([R.chain(m)[1] for m in msgs]))


@pytest.mark.parametrize("case", ["empty", "five"])
def test_gpu_proof_over_device_tables_is_the_oracles(gpu, case):
    msgs = [b""] if case == "empty" else R.set_12131()
    over = dict(queries=4, pow_bits=2)
    try:
        blob = gpu.set_params(1, **over)
        o.oracle_set_params(1, **over)
        proof, digests, tables = S.prove_keccak256(gpu, msgs, params=blob)
        assert digests == [keccak.keccak256(m) for m in msgs]
        rows = R.sponge_rows(msgs)
        n_blocks = int(rows[:, L.REAL].sum()) // 3
        host = [p3.Table.from_canonical(tables[0].air, rows), p3.Table.from_canonical(tables[1].air, CR.chip_rows(R.states_of(rows, n_blocks)[0]))]
        init, _claims = S.statement(msgs, digests)
        assert np.array_equal(proof, o.oracle_p3_prove(host, init))    # the oracle proves the numpy rows: this holds the device rows too
        assert S.verify_keccak256(msgs, digests, proof, params=blob) == 0
        if case == "five":                                             # one bit of the second message's second block
            flipped = [msgs[0], msgs[1][:150] + bytes([msgs[1][150] ^ 0x10]) + msgs[1][151:]] + msgs[2:]
        else:                                                          # the empty message has no bit: one zero byte, still one block
            flipped = [b"\x00"]
        assert S.verify_keccak256(flipped, digests, proof, params=blob) == 8
    finally:
        o.oracle_set_params()
        gpu.set_params(1)


def test_gpu_refusals_leave_the_context_usable(gpu):
    lib = _lib.load()
    msgs = [b"abc", bytes(200)]
    blocks, first = S.pad_blocks(msgs)
    d_blocks, d_first = gpu.copy_from_elem(blocks.view(np.uint32).reshape(-1)), gpu.copy_from_elem(first)
    d_rows, d_st, d_out, d_dig = gpu.alloc_elem(16 * L.WIDTH), gpu.alloc_elem(3 * 50), gpu.alloc_elem(3 * 50), gpu.alloc_elem(2 * 8)
    good = dict(ctx=gpu._ctx, b=d_blocks.ptr, f=d_first.ptr, k=2, nb=3, rows=16, t=d_rows.ptr, s=d_st.ptr, o=d_out.ptr, d=d_dig.ptr)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rk_keccak_sponge_trace(a["ctx"], a["b"], a["f"], None, a["k"], a["nb"], a["rows"], a["t"], a["s"], a["o"], a["d"])

    for name in ("ctx", "b", "f", "t", "s", "o", "d"):
        assert call(**{name: None}) == _lib.RK_ERR_INVALID, name
    assert call(k=0) == _lib.RK_ERR_INVALID and call(nb=0) == _lib.RK_ERR_INVALID
    assert call(k=4) == _lib.RK_ERR_INVALID                            # more messages than blocks
    assert call(rows=12) == _lib.RK_ERR_INVALID                        # no power of two
    assert call(rows=8) == _lib.RK_ERR_INVALID                         # below 3 n_blocks
    assert call(k=1, nb=1, rows=1) == _lib.RK_ERR_INVALID
    assert call(rows=1 << 25) == _lib.RK_ERR_INVALID                   # above 2^24
    assert call() == 0
    assert np.array_equal(d_rows.to_host().reshape(16, L.WIDTH), p3.to_mont(R.sponge_rows(msgs)))
    assert S.digest_bytes(d_dig.to_host().view(np.uint64).reshape(2, 4)) == [keccak.keccak256(m) for m in msgs]
