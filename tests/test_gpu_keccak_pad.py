"""The Keccak-256 padding table on the GPU (rk_keccak_pad_trace / rk_keccak_pad_digests, keccak_pad.hip;
raiko_amd/keccak_pad.py): the rows the kernels write equal the numpy restatement (tests/keccak_pad_ref.py) and the blocks
equal keccak_sponge.pad_blocks word for word at every launch threshold -- the empty message, a tail past three bytes, the
pad byte 0x81, a block of padding alone, a thread block of either kernel full and the first second one, a nine-block
message, a table half of whose slots are padding, given message IDs --, the bytes past a message's end change W and its
bits and nothing else, the sponge's and the chip's rows over the device-padded blocks are their own restatements, a proof
over the three device tables equals the oracle's over the restatements', verify_keccak256_words accepts it and refuses a
flipped bit and a length off by one, and the refusals leave the context usable."""
import numpy as np
import pytest

import keccak_chip_ref as CR
import keccak_pad_ref as R
import keccak_sponge_ref as SR
import oracle_lib as o
from raiko_amd import _lib, hal, keccak, keccak_chip as K, keccak_pad as KP, keccak_sponge as S, p3

pytestmark = pytest.mark.gpu

L = KP.Layout
CASES = R.kernel_cases()


@pytest.fixture(scope="module")
def gpu():
    h = hal.HipHal(0)
    yield h
    h.close()


@pytest.mark.parametrize("name", list(CASES))
def test_gpu_rows_and_blocks_equal_the_restatement(gpu, name):
    msgs, ids, rows, tail = CASES[name]
    t = KP.keccak_pad_trace(gpu, msgs, None if ids is None else p3.to_mont(ids), rows, tail)
    blocks, first = S.pad_blocks(msgs)
    assert t.n_blocks == blocks.shape[0] and t.rows == (KP.min_rows(t.n_blocks) if rows is None else rows)
    assert np.array_equal(t.blocks(), blocks)
    assert np.array_equal(t.d_rows.to_host().reshape(t.rows, L.WIDTH), p3.to_mont(R.pad_rows(msgs, ids, rows, tail, digests=False)))
    digs = np.frombuffer(b"".join(keccak.keccak256(m) for m in msgs), dtype="<u8").copy()
    KP.put_digests(gpu, t, gpu.copy_from_elem(digs.view(np.uint32)))
    assert np.array_equal(t.d_rows.to_host().reshape(t.rows, L.WIDTH), p3.to_mont(R.pad_rows(msgs, ids, rows, tail)))


def test_gpu_tail_bytes_reach_w_and_nothing_else(gpu):
    msgs = [bytes(range(1, 8)), bytes(range(9, 150))]                  # 7 = 4 + 3 and 141 = 4 x 35 + 1 bytes
    a = KP.keccak_pad_trace(gpu, msgs, tail=[b"\x00", b"\x00\x00\x00"])
    b = KP.keccak_pad_trace(gpu, msgs, tail=[b"\xff", b"\x80\x01\xfe"])
    assert np.array_equal(a.blocks(), b.blocks()) and np.array_equal(a.blocks(), S.pad_blocks(msgs)[0])
    ra, rb = (t.d_rows.to_host().reshape(t.rows, L.WIDTH) for t in (a, b))
    differ = np.argwhere(ra != rb)
    assert sorted(set(differ[:, 0].tolist())) == [1, 34 + 35]          # the two END rows
    assert set(differ[:, 1].tolist()) <= {L.W_LO, L.W_HI} | set(range(L.WB, L.WB + 32)) and L.W_HI in differ[:, 1]


def test_gpu_sponge_and_chip_rows_over_device_padded_blocks(gpu):
    msgs = SR.set_12131()
    pad, sponge, chip = KP.keccak_pad_tables(gpu, msgs, tail=[b"\x11\x22", b"", b"\x33", b"", b""])
    st = sponge.trace_info
    assert (pad.device[1], sponge.device[1], chip.device[1]) == (9, 5, 8) and st.n_blocks == 8 == pad.trace_info.n_blocks
    assert np.array_equal(pad.device[0].to_host().reshape(512, L.WIDTH), p3.to_mont(R.pad_rows(msgs, tail=[b"\x11\x22", b"", b"\x33", b"", b""])))
    assert np.array_equal(sponge.device[0].to_host().reshape(32, S.Layout.WIDTH), p3.to_mont(SR.sponge_rows(msgs)))
    assert np.array_equal(chip.device[0].to_host().reshape(256, K.Layout.WIDTH), p3.to_mont(CR.chip_rows(st.states)))
    assert np.array_equal(st.states, np.concatenate([SR.chain(m)[1] for m in msgs]))
    assert S.digest_bytes(st.digests) == [keccak.keccak256(m) for m in msgs]


@pytest.mark.parametrize("case", ["empty", "five"])
def test_gpu_proof_over_device_tables_is_the_oracles(gpu, case):
    msgs = [b""] if case == "empty" else SR.set_12131()
    tail = None if case == "empty" else [b"\x11\x22", b"", b"\x33", b"", b""]
    over = dict(queries=4, pow_bits=2)
    try:
        blob = gpu.set_params(1, **over)
        o.oracle_set_params(1, **over)
        proof, digests, tables = KP.prove_keccak256_words(gpu, msgs, params=blob, tail=tail)
        assert digests == [keccak.keccak256(m) for m in msgs]
        sponge_rows = SR.sponge_rows(msgs)
        n_blocks = int(sponge_rows[:, S.Layout.REAL].sum()) // 3
        host = [p3.Table.from_canonical(tables[0].air, R.pad_rows(msgs, tail=tail)), p3.Table.from_canonical(tables[1].air, sponge_rows),
                p3.Table.from_canonical(tables[2].air, CR.chip_rows(SR.states_of(sponge_rows, n_blocks)[0]))]
        init, _claims = KP.statement_words(msgs, digests, tail=tail)
        assert np.array_equal(proof, o.oracle_p3_prove(host, init))    # the oracle proves the numpy rows: this holds the device rows too
        assert KP.verify_keccak256_words(msgs, digests, proof, params=blob, tail=tail) == 0
        if case == "five":
            flipped = [msgs[0], msgs[1][:150] + bytes([msgs[1][150] ^ 0x10]) + msgs[1][151:]] + msgs[2:]
            assert KP.verify_keccak256_words(flipped, digests, proof, params=blob, tail=tail) == 8
            # a length off by one in the same word, every word claim unchanged: message 0 as 11 bytes, 0x11 taken in
            longer, rest = [msgs[0] + b"\x11"] + msgs[1:], [b"\x22"] + tail[1:]
            assert KP.words_of(longer, rest)[0].tolist() == KP.words_of(msgs, tail)[0].tolist()
            assert KP.verify_keccak256_words(longer, digests, proof, params=blob, tail=rest) == 8
        else:                                                          # the empty message has no bit and no word: one zero byte
            assert KP.verify_keccak256_words([b"\x00"], digests, proof, params=blob) == 8
    finally:
        o.oracle_set_params()
        gpu.set_params(1)


def test_gpu_refusals_leave_the_context_usable(gpu):
    lib = _lib.load()
    msgs, tail = [b"abc", bytes(200)], [b"\x7f", b""]
    words, word_first, lens, first = KP.words_of(msgs, tail)
    d_words, d_wf, d_lens, d_first = (gpu.copy_from_elem(a) for a in (words, word_first, lens, first))
    d_rows, d_blocks = gpu.alloc_elem(128 * L.WIDTH), gpu.alloc_elem(3 * 34)
    d_dig = gpu.copy_from_elem(np.frombuffer(b"".join(keccak.keccak256(m) for m in msgs), dtype="<u4").copy())
    good = dict(ctx=gpu._ctx, w=d_words.ptr, wf=d_wf.ptr, l=d_lens.ptr, f=d_first.ptr, k=2, nb=3, rows=128, t=d_rows.ptr, b=d_blocks.ptr, d=d_dig.ptr)

    def call(**kw):
        a = dict(good, **kw)
        return lib.rk_keccak_pad_trace(a["ctx"], a["w"], words.size, a["wf"], a["l"], a["f"], None, a["k"], a["nb"], a["rows"], a["t"], a["b"])

    def digests(**kw):
        a = dict(good, **kw)
        return lib.rk_keccak_pad_digests(a["ctx"], a["d"], a["f"], a["k"], a["nb"], a["rows"], a["t"])

    for name in ("ctx", "w", "wf", "l", "f", "t", "b"):
        assert call(**{name: None}) == _lib.RK_ERR_INVALID, name
    for name in ("ctx", "d", "f", "t"):
        assert digests(**{name: None}) == _lib.RK_ERR_INVALID, name
    for fn in (call, digests):
        assert fn(k=0) == _lib.RK_ERR_INVALID
        assert fn(k=4) == _lib.RK_ERR_INVALID                          # more messages than blocks
        assert fn(rows=96) == _lib.RK_ERR_INVALID                      # no power of two
        assert fn(rows=64) == _lib.RK_ERR_INVALID                      # below 34 n_blocks
        assert fn(rows=1 << 25) == _lib.RK_ERR_INVALID                 # above 2^24
    assert call() == 0
    assert np.array_equal(d_blocks.to_host().view(np.uint64).reshape(3, 17), S.pad_blocks(msgs)[0])
    assert np.array_equal(d_rows.to_host().reshape(128, L.WIDTH), p3.to_mont(R.pad_rows(msgs, tail=tail, digests=False)))
    assert digests() == 0
    assert np.array_equal(d_rows.to_host().reshape(128, L.WIDTH), p3.to_mont(R.pad_rows(msgs, tail=tail)))
