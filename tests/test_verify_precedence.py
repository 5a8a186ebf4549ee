"""A seal with two defects gets the reason code of the check that comes first in rk_verify_segment_ex: every word < p,
then the header, the commitments, proof of work, and the queries in order, with trailing words last.  The expected
codes are what the verifier returned before it was cut into stages."""
import numpy as np
import pytest

import oracle_lib as o
from raiko_amd import hal
from raiko_amd.segment import synthetic_segment

P = o.P
WIDTHS = (4, 4, 20)


def seal_layout(seg, seal, queries, blow, fold_log2, min_degree, pow_bits):
    """word offsets of a seal's parts, from the proof's shape written out here on its own"""
    n = 1 << seg.po2
    fold = 1 << fold_log2

    def cap(rows):   # digests of a tree's top layer: the largest layer below the leaves that is no wider than `queries`
        layers = rows.bit_length() - 1
        return 8 << max([0] + [i for i in range(1, layers) if (1 << i) <= queries])

    at = {"po2": seg.globals_.size}
    pos = seg.globals_.size + 1 + 4 * cap(n << blow)
    pos += 4 * (seg.taps.tot_taps + (4 << blow))
    size = n
    rounds = 0
    while size > min_degree and size >= fold:
        pos += cap((size << blow) // fold)
        size //= fold
        rounds += 1
    pos += 4 * size
    if pow_bits:
        at["nonce"] = pos
        pos += 1
    at["query0"] = pos                                   # the accum row of the first query
    at["rounds"] = rounds
    at["last"] = seal.size - 1                           # a digest of the last query's last FRI opening
    return at


def bump(seal, *offsets):
    bad = seal.copy()
    for off in offsets:
        bad[off] = (int(bad[off]) + 1) % P
    return bad


@pytest.fixture(scope="module")
def risc0_seal():
    seg = synthetic_segment(9, WIDTHS, seed=909)         # degree 512: one FRI round under risc0's shape
    seal = o.oracle_prove(seg)
    at = seal_layout(seg, seal, 50, 2, 4, 256, 0)
    assert at["rounds"] == 1 and hal.verify_segment(seg, seal) == 0
    return seg, seal, at


def test_single_defects(risc0_seal):
    seg, seal, at = risc0_seal
    assert hal.verify_segment(seg, bump(seal, at["po2"])) == 10
    assert hal.verify_segment(seg, bump(seal, at["query0"])) == 20
    assert hal.verify_segment(seg, bump(seal, at["last"])) == 30
    assert hal.verify_segment(seg, seal[:-1]) == 60
    assert hal.verify_segment(seg, np.concatenate([seal, seal[:1]])) == 61
    big = seal.copy()
    big[at["last"]] += P
    assert hal.verify_segment(seg, big) == 63


# expected codes: returned by the library built from commit aac9052 (the one-function verify_segment)
def test_non_canonical_word_before_a_bad_header(risc0_seal):
    seg, seal, at = risc0_seal
    bad = bump(seal, at["po2"])
    bad[at["last"]] += P                                 # the last word of the seal: found before anything is hashed
    assert hal.verify_segment(seg, bad) == 63


def test_bad_header_before_a_truncation(risc0_seal):
    seg, seal, at = risc0_seal
    assert hal.verify_segment(seg, bump(seal, at["po2"])[:-100]) == 10
    assert hal.verify_segment(seg, bump(seal, 3)[: seal.size // 2]) == 10     # a global instead of po2
    assert hal.verify_segment(seg, seal[: at["po2"]]) == 10                   # cut inside the header itself


def test_broken_group_opening_before_a_trailing_word(risc0_seal):
    seg, seal, at = risc0_seal
    bad = np.concatenate([bump(seal, at["query0"] + WIDTHS[0] + 1), seal[:1]])   # a digest of the accum path, query 0
    assert hal.verify_segment(seg, bad) == 20
    bad = np.concatenate([bump(seal, at["last"]), seal[:1]])
    assert hal.verify_segment(seg, bad) == 30


def test_proof_of_work_before_the_fri_openings_under_sp1():
    """the nonce and a word of a FRI round's opened coset (on its own a failed round opening: an inconsistent fold behind
    a valid path would need the round's tree hashed again)"""
    o.oracle_set_params(1)
    try:
        seg = synthetic_segment(9, WIDTHS, seed=910, blowup_log2=1)
        seal = o.oracle_prove(seg)
    finally:
        o.oracle_set_params()
    blob = hal.make_params(1)
    at = seal_layout(seg, seal, blob.queries, blob.blowup_log2, blob.fri_fold_log2, blob.fri_min_degree, blob.pow_bits)
    assert blob.pow_bits and at["rounds"] > 1
    assert hal.verify_segment(seg, seal, params=blob) == 0
    assert hal.verify_segment(seg, bump(seal, at["nonce"]), params=blob) == 62
    assert hal.verify_segment(seg, bump(seal, at["last"]), params=blob) == 30 + min(at["rounds"] - 1, 9)
    assert hal.verify_segment(seg, bump(seal, at["nonce"], at["last"]), params=blob) == 62
    assert hal.verify_segment(seg, bump(seal, at["nonce"])[:-1], params=blob) == 62
