"""The per-device cache of the committed code group (raiko_amd/csrc/code_cache.hip): a proof that finds the code
group of its input in the cache borrows coefficients, LDE, Merkle tree and top layer instead of computing them, and
its seal is word for word the oracle's all the same.  The cache goes by contents, never by address: every variant of
an input that differs in one word, or in the order of two, misses; the same words at another address hit.

All comparisons are exact (seals against oracle_lib.oracle_prove, counters against the counts the policy implies), so
there is no tolerance anywhere in this file.  Shapes: widths 16 / 16 / 32 at po2 8 (a code group of exactly one
4096-word fingerprint chunk) and po2 12 (16 chunks, one block each); the toy circuit's 4 x 2^9 code group is a partial chunk."""
import functools

import numpy as np
import pytest

import oracle_lib as o
from raiko_amd import _lib, hal as halmod
from raiko_amd.hal import HipHal, prove_session, verify_segment
from raiko_amd.segment import P, Segment, synthetic_segment

gpu = pytest.mark.gpu
WIDTHS = (16, 16, 32)
DEFAULT_BYTES = 2 << 30
SEED_A, SEED_B = 501, 777


def entry_bytes(po2, cols, blowup_log2=2):
    """device bytes of one entry: coefficients + LDE + the Merkle heap of 2 * rows digests"""
    n = 1 << po2
    d = n << blowup_log2
    return cols * n * 4 + cols * d * 4 + 2 * d * 32


@functools.lru_cache(maxsize=None)
def ref(po2, seed):
    """(segment, the oracle's seal): computed once, shared by every test, never modified"""
    seg = synthetic_segment(po2, WIDTHS, seed=seed)
    for g in seg.groups:
        g.setflags(write=False)
    want = o.oracle_prove(seg)
    want.setflags(write=False)
    return seg, want


def with_code(seg, code):
    return Segment(po2=seg.po2, taps=seg.taps, groups=[seg.groups[0], code, seg.groups[2]], check=seg.check, globals_=seg.globals_)


class Counters:
    def __init__(self, device=0):
        self.device = device
        self.base = halmod.code_cache_stats(device)

    def delta(self):
        now = halmod.code_cache_stats(self.device)
        return now["hits"] - self.base["hits"], now["misses"] - self.base["misses"]

    def bytes(self):
        return halmod.code_cache_stats(self.device)["bytes"]


@pytest.fixture()
def cache():
    """an empty cache of the default size; the default again afterwards"""
    halmod.code_cache_configure(0, 0)
    halmod.code_cache_configure(0, DEFAULT_BYTES)
    yield Counters()
    halmod.code_cache_configure(0, 0)
    halmod.code_cache_configure(0, DEFAULT_BYTES)


def device_inputs(hal, seg):
    return [hal.copy_from_elem(g) for g in seg.groups], hal.copy_from_elem(seg.check)


def prove(hal, seg, on_device):
    """one proof with the inputs where `on_device` says; for 2 also: the code buffer comes back untouched"""
    if on_device == 0:
        return hal.prove_segment(seg)
    groups, check = device_inputs(hal, seg)
    seal = hal.prove_segment(seg, device_inputs=(groups, check), consume_inputs=on_device == 2)
    assert np.array_equal(groups[1].to_host().reshape(seg.groups[1].shape), seg.groups[1])
    return seal


def test_controls_need_no_gpu():
    lib = _lib.load()
    assert lib.rk_code_cache_configure(-1, 0) == _lib.RK_ERR_INVALID
    assert lib.rk_code_cache_stats(-1, None, None, None) == _lib.RK_ERR_INVALID
    assert lib.rk_code_cache_stats(0, None, None, None) == 0
    before = halmod.code_cache_stats(63)
    assert before["bytes"] == 0
    halmod.code_cache_configure(63, 12345)
    halmod.code_cache_configure(63, 0)
    assert halmod.code_cache_stats(63) == before
    assert lib.rk_session_release() == 0


@gpu
@pytest.mark.parametrize("on_device", [0, 1, 2])
@pytest.mark.parametrize("po2", [8, 12])
def test_a_b_a_b_two_misses_two_hits(hal, cache, po2, on_device):
    held = []
    for i, seed in enumerate((SEED_A, SEED_B, SEED_A, SEED_B)):
        seg, want = ref(po2, seed)
        got = prove(hal, seg, on_device)
        assert got.size == want.size and np.array_equal(got, want), i
        assert verify_segment(seg, got) == 0
        held.append(cache.bytes())
    assert cache.delta() == (2, 2)
    assert held == [entry_bytes(po2, 16), 2 * entry_bytes(po2, 16)] + [2 * entry_bytes(po2, 16)] * 2


@gpu
@pytest.mark.parametrize("po2", [8, 12])
def test_cache_off_same_seals_no_hits(hal, po2):
    base = Counters()
    halmod.code_cache_configure(0, 0)
    try:
        for seed in (SEED_A, SEED_B, SEED_A, SEED_B):
            seg, want = ref(po2, seed)
            assert np.array_equal(hal.prove_segment(seg), want)
            groups, check = device_inputs(hal, seg)
            assert np.array_equal(hal.prove_segment(seg, device_inputs=(groups, check)), want)
        assert base.delta() == (0, 0) and base.bytes() == 0
    finally:
        halmod.code_cache_configure(0, DEFAULT_BYTES)


@gpu
@pytest.mark.parametrize("po2", [8, 12])
def test_contents_decide_not_the_address(hal, cache, po2):
    seg, want = ref(po2, SEED_A)
    code = seg.groups[1]
    last = code.copy()
    last[-1, -1] = (int(last[-1, -1]) + 1) % P
    first = code.copy()
    first[0, 0] = (int(first[0, 0]) + 1) % P
    swapped = code.copy()
    i, j = 3, (1 << po2) - 5
    assert swapped[7, i] != swapped[7, j]
    swapped[7, i], swapped[7, j] = code[7, j], code[7, i]
    groups, check = device_inputs(hal, seg)
    assert np.array_equal(hal.prove_segment(seg, device_inputs=(groups, check)), want)
    assert cache.delta() == (0, 1)
    for k, variant in enumerate((last, first, swapped)):
        vseg = with_code(seg, variant)
        groups[1].copy_from(variant)              # the same device address, other contents
        got = hal.prove_segment(vseg, device_inputs=(groups, check))
        assert cache.delta() == (0, 2 + k)
        assert np.array_equal(got, o.oracle_prove(vseg)) and not np.array_equal(got, want)
    elsewhere = hal.copy_from_elem(code)          # groups[1] is still allocated: another address
    assert elsewhere.ptr != groups[1].ptr
    got = hal.prove_segment(seg, device_inputs=([groups[0], elsewhere, groups[2]], check))
    assert cache.delta() == (1, 4)
    assert np.array_equal(got, want)


@gpu
def test_a_word_that_is_no_field_element_bypasses_the_cache(hal, cache):
    """m and m + p agree mod p, so the fingerprint has no collision bound for words >= p: such an input is committed the
    ordinary way, twice if it comes twice, and the seal is the one the build without a cache gives"""
    seg, _ = ref(8, SEED_A)
    code = seg.groups[1].copy()
    code[5, 9] = np.uint32(int(code[5, 9]) + P)
    vseg = with_code(seg, code)
    a = hal.prove_segment(vseg)
    b = hal.prove_segment(vseg)
    assert cache.delta() == (0, 0) and cache.bytes() == 0
    halmod.code_cache_configure(0, 0)
    assert np.array_equal(a, b) and np.array_equal(a, hal.prove_segment(vseg))


@gpu
def test_parameters_and_shape_are_part_of_the_key(cache):
    h = HipHal(0)
    try:
        seg, want = ref(12, SEED_A)
        assert np.array_equal(h.prove_segment(seg), want)
        assert cache.delta() == (0, 1)
        # the same code columns under SP1's set: blow-up 2, Poseidon2 width 16, another field and query count
        sp1 = synthetic_segment(12, WIDTHS, seed=SEED_A, blowup_log2=1)
        assert np.array_equal(sp1.groups[1], seg.groups[1])
        o.oracle_set_params(1)
        blob = h.set_params(1)
        got = h.prove_segment(sp1)
        assert cache.delta() == (0, 2)
        assert np.array_equal(got, o.oracle_prove(sp1)) and verify_segment(sp1, got, params=blob) == 0
        assert cache.bytes() == entry_bytes(12, 16) + entry_bytes(12, 16, 1)
        o.oracle_set_params()
        h.set_params(0)
        assert np.array_equal(h.prove_segment(seg), want)
        assert cache.delta() == (1, 2)
        # the words of a po2-9 code group again at po2 8 as twice the columns: the key holds po2 and the column count
        seg9, want9 = ref(9, SEED_A)
        assert np.array_equal(h.prove_segment(seg9), want9)
        assert cache.delta() == (1, 3)
        base = synthetic_segment(8, (16, 32, 32), seed=SEED_B)
        wide = Segment(po2=8, taps=base.taps, groups=[base.groups[0], np.ascontiguousarray(seg9.groups[1]).reshape(32, 256),
                                                      base.groups[2]], check=base.check, globals_=base.globals_)
        assert wide.groups[1].tobytes() == seg9.groups[1].tobytes()
        got = h.prove_segment(wide)
        assert cache.delta() == (1, 4)
        assert np.array_equal(got, o.oracle_prove(wide))
    finally:
        o.oracle_set_params()
        h.close()


@gpu
@pytest.mark.parametrize("po2", [8, 12])
def test_room_for_one_entry_evicts(hal, po2):
    limit = entry_bytes(po2, 16)
    base = Counters()
    halmod.code_cache_configure(0, 0)
    halmod.code_cache_configure(0, limit)
    try:
        for k, seed in enumerate((SEED_A, SEED_B, SEED_A)):
            seg, want = ref(po2, seed)
            assert np.array_equal(hal.prove_segment(seg), want)
            assert base.delta() == (0, k + 1)
            assert base.bytes() == limit
        halmod.code_cache_configure(0, limit - 1)      # no entry fits: off for this shape, nothing held
        assert base.bytes() == 0
        seg, want = ref(po2, SEED_A)
        assert np.array_equal(hal.prove_segment(seg), want)
        assert base.delta() == (0, 3) and base.bytes() == 0
    finally:
        halmod.code_cache_configure(0, 0)
        halmod.code_cache_configure(0, DEFAULT_BYTES)


@gpu
def test_session_three_in_flight(cache):
    refs = [ref(12, SEED_A), ref(12, SEED_B)]
    segs = [refs[i % 2][0] for i in range(12)]
    seals = prove_session(segs, inflight=3, upload_ahead=2, verify=True)
    for i, seal in enumerate(seals):
        assert np.array_equal(seal, refs[i % 2][1]), i
    hits, misses = cache.delta()
    assert hits + misses == 12
    assert 2 <= misses <= 2 * 3         # at worst every context misses once per key: duplicates are dropped, not awaited
    assert cache.bytes() == 2 * entry_bytes(12, 16)
    halmod.session_release()
    assert cache.bytes() == 0           # rk_session_release drops the cache too
    seals = prove_session(segs[:2], inflight=1, verify=True)
    assert np.array_equal(seals[0], refs[0][1]) and np.array_equal(seals[1], refs[1][1])
    h = HipHal(0)                       # entries belong to the device: a context that has never seen the input hits
    try:
        before = cache.delta()
        assert np.array_equal(h.prove_segment(refs[0][0]), refs[0][1])
        assert cache.delta() == (before[0] + 1, before[1])
    finally:
        h.close()


@gpu
def test_toy_circuit_behind_hooks(hal, cache):
    from raiko_amd import toy_circuit
    toy_circuit.load()
    seg = toy_circuit.toy_segment(9, (8, 4, 8), seed=109)
    want = o.oracle_prove(seg)
    first = hal.prove_segment(seg)
    assert cache.delta() == (0, 1)
    second = hal.prove_segment(seg)
    assert cache.delta() == (1, 1)
    assert np.array_equal(first, want) and np.array_equal(second, want)
    for seal in (first, second):
        assert verify_segment(seg, seal, poly_ext=toy_circuit.poly_ext_fn()) == 0
        assert o.oracle_verify(seg, seal, toy_identity=True) == 0
    # the raw code witness reaches `accumulate` from device-resident inputs as well, hit or not
    groups = [None, hal.copy_from_elem(seg.groups[1]), hal.copy_from_elem(seg.groups[2])]
    assert np.array_equal(hal.prove_segment(seg, device_inputs=(groups, None)), want)
    assert np.array_equal(hal.prove_segment(seg, device_inputs=(groups, None), consume_inputs=True), want)
    assert cache.delta() == (3, 1)
