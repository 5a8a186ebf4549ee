"""code_fingerprint_kernel (raiko_amd/csrc/code_cache.hip) decides whether a proof borrows a cached commitment of its
code group.  It can be observed only through rk_code_cache_stats and the seal, and that is enough: a variant of a cached
input must MISS and give the oracle's seal of the variant; the same words anywhere else must HIT and give the cached
input's seal.  A fingerprint that ignored part of its input would hit on a variant in that part and hand back the base
seal.

Shapes (threshold_cases; tests/test_launch_thresholds.py proves where they lie): S1, 4 352 words, a whole chunk beside
a partial one; S2, 1 028 chunks on 1 024 workgroups, so that workgroups 0..3 loop to a second chunk; S3, the same words
at an address one word past a 16-byte boundary, where the kernel loads word by word instead of by uint4.  Every variant
is uploaded into the same device buffer, so the address never changes.  All comparisons are exact."""
import functools

import numpy as np
import pytest

import oracle_lib as o
import threshold_cases as T
from raiko_amd import hal as halmod
from raiko_amd.hal import verify_segment
from raiko_amd.segment import P, synthetic_segment
from test_gpu_code_cache import cache, with_code  # noqa: F401  (cache: the fixture, an empty cache and its Counters)

gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def ref(shape):
    """(segment, the oracle's seal): computed once, shared by every test, never modified"""
    po2, widths, seed = shape
    seg = synthetic_segment(po2, widths, seed=seed)
    for g in seg.groups:
        g.setflags(write=False)
    want = o.oracle_prove(seg)
    want.setflags(write=False)
    return seg, want


class Proven:
    """the base input of `shape` on the device, proven once: one miss, the oracle's seal"""

    def __init__(self, hal, cache, shape):
        self.hal, self.cache = hal, cache
        self.seg, self.want = ref(shape)
        self.code = self.seg.groups[1]
        self.groups = [hal.copy_from_elem(g) for g in self.seg.groups]
        self.check = hal.copy_from_elem(self.seg.check)
        self.hits, self.misses = 0, 0
        got = self.prove(self.code)
        self.expect(miss=True)
        assert np.array_equal(got, self.want)

    def prove(self, code, at=None):
        """the proof of the segment with `code` as its code group, uploaded into the one device buffer (or read at `at`)"""
        if at is None:
            self.groups[1].copy_from(code)
            at = self.groups[1]
        return self.hal.prove_segment(with_code(self.seg, code), device_inputs=([self.groups[0], at, self.groups[2]], self.check))

    def expect(self, miss):
        self.hits, self.misses = self.hits + (not miss), self.misses + bool(miss)
        assert self.cache.delta() == (self.hits, self.misses)

    def variant_misses(self, code, oracle=True):
        assert not np.array_equal(code, self.code)
        got = self.prove(code)
        self.expect(miss=True)
        vseg = with_code(self.seg, code)
        if oracle:
            assert np.array_equal(got, o.oracle_prove(vseg))
        else:
            assert verify_segment(vseg, got) == 0
        assert got.size == self.want.size and not np.array_equal(got, self.want)

    def base_hits_again(self):
        got = self.prove(self.code)
        self.expect(miss=False)
        assert np.array_equal(got, self.want)


# ---- 1. every register slot of a lane: a[4 q + e], w[4 q + e] ----
@gpu
@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_one_word_of_every_lane_slot_misses(hal, cache, q):
    s = Proven(hal, cache, T.S1)
    for e in range(4):
        for t in T.SLOT_LANES:
            s.variant_misses(T.bumped(s.code, T.chunk_slot(t, q, e)))
    s.base_hits_again()


@gpu
def test_one_word_of_the_partial_chunk_misses(hal, cache):
    s = Proven(hal, cache, T.S1)
    for e in range(4):
        for t in (0, 63):
            s.variant_misses(T.bumped(s.code, T.CHUNK + T.chunk_slot(t, 0, e)))
    s.base_hits_again()


# ---- 2. a word in a chunk of the first and of the second pass of the strided loop ----
@gpu
def test_one_word_in_either_pass_of_the_chunk_loop_misses(hal, cache):
    s = Proven(hal, cache, T.S2)
    words = s.code.size
    for i in T.S2_PASS_INDICES:
        s.variant_misses(T.bumped(s.code, i % words), oracle=i in T.S2_ORACLE_INDICES)
    s.base_hits_again()


# ---- 3. the same multiset of words in another order ----
@gpu
def test_two_words_of_one_lane_swapped_miss(hal, cache):
    s = Proven(hal, cache, T.S1)
    i = T.chunk_slot(70, 2, 1)
    s.variant_misses(T.swapped(s.code, i, i + 1))
    s.base_hits_again()


@gpu
def test_words_and_chunks_swapped_across_the_chunk_loop_miss(hal, cache):
    s = Proven(hal, cache, T.S2)
    i, k = 5 * T.CHUNK + T.chunk_slot(129, 3, 2), T.chunk_slot(200, 1, 3)
    s.variant_misses(T.swapped(s.code, i, i + T.CHUNK), oracle=False)                       # one slot, neighbouring chunks
    s.variant_misses(T.swapped(s.code, 3 * T.CHUNK + k, 1027 * T.CHUNK + k), oracle=False)  # one slot of one workgroup, successive iterations
    s.variant_misses(T.swapped(s.code, 0, 1024 * T.CHUNK, n=T.CHUNK))                       # workgroup 0's two chunks exchanged
    s.base_hits_again()


# ---- 4. a word >= p: no collision bound, so no cache ----
def ge_p(code, index):
    out = code.copy()
    flat = out.reshape(-1)
    flat[index] = np.uint32(int(flat[index]) + P)
    return out


def offset_copy(hal, code):
    """(buffer, address): the words of `code` from one word past a 16-byte boundary on"""
    host = np.zeros(code.size + 4, dtype=np.uint32)
    host[1: 1 + code.size] = code.reshape(-1)
    buf = hal.copy_from_elem(host)
    assert buf.ptr % 16 == 0
    return buf, buf.ptr + 4


@gpu
@pytest.mark.parametrize("shape,index,offset", [(T.S1, T.CHUNK + T.chunk_slot(17, 0, 2), False), (T.S2, 1027 * T.CHUNK + T.chunk_slot(255, 3, 3), False),
                                                (T.S3_SHAPES[1], 9 * T.CHUNK + T.chunk_slot(64, 1, 0), True)],
                         ids=["S1-partial-chunk", "S2-chunk-1027", "S3-offset-address"])
def test_a_word_that_is_no_field_element_bypasses_the_cache(hal, cache, shape, index, offset):
    po2, widths, seed = shape
    seg = synthetic_segment(po2, widths, seed=seed)
    code = ge_p(seg.groups[1], index)
    vseg = with_code(seg, code)
    groups, check = [hal.copy_from_elem(g) for g in vseg.groups], hal.copy_from_elem(seg.check)
    if offset:
        keep, groups[1] = offset_copy(hal, code)
    a = hal.prove_segment(vseg, device_inputs=(groups, check))
    b = hal.prove_segment(vseg, device_inputs=(groups, check))
    assert cache.delta() == (0, 0) and cache.bytes() == 0
    halmod.code_cache_configure(0, 0)
    assert np.array_equal(a, b) and np.array_equal(a, hal.prove_segment(vseg, device_inputs=(groups, check)))
    assert verify_segment(vseg, a) == 0


# ---- 5. the uint4 loads and the word-by-word loads give one fingerprint ----
@gpu
@pytest.mark.parametrize("shape", T.S3_SHAPES, ids=["S1", "po2-12"])
def test_the_two_load_paths_agree(hal, cache, shape):
    s = Proven(hal, cache, shape)                       # from an aligned buffer: a miss
    assert s.groups[1].ptr % 16 == 0
    buf, addr = offset_copy(hal, s.code)
    got = s.prove(s.code, at=addr)                      # the same words, read word by word: a hit
    s.expect(miss=False)
    assert np.array_equal(got, s.want)
    chunks = s.code.size // T.CHUNK
    for index in ((chunks - 1) * T.CHUNK + T.chunk_slot(63, 2, 3), s.code.size - 1):     # a whole chunk's word; the last word
        variant = T.bumped(s.code, index)
        host = np.zeros(s.code.size + 4, dtype=np.uint32)
        host[1: 1 + s.code.size] = variant.reshape(-1)
        buf.copy_from(host)
        got = s.prove(variant, at=addr)
        s.expect(miss=True)
        assert np.array_equal(got, o.oracle_prove(with_code(s.seg, variant))) and not np.array_equal(got, s.want)
        again = s.prove(variant)                        # the variant from the aligned buffer: the entry just made
        s.expect(miss=False)
        assert np.array_equal(again, got)
    s.base_hits_again()
