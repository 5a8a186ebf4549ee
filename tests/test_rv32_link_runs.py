"""Linked rv32im-mem runs over many shards and under other parameter sets, on the CPU: the `relay` guest of
tests/rv32_link_programs.py (five shards; words whose histories skip shards; a shard that touches nothing) through
rv32link.check_memory_chain against the plain-Python replay, forged journal rows that only a chain remembering every
earlier shard refuses, rv32link.airs / rv32mem.airs built for the other extension (x^4 + 11) on every shard, and
rk_rv32mem_journal_root against the oracle's MMCS root under every parameter set whose hash differs (SP1's width-16
Poseidon2, risc0's width-24 sponge, custom round-constant tables) and one whose hash does not (risc0's field under
SP1's hash).  Every comparison is bit-exact."""
import numpy as np
import pytest

import fri_param_sets as PS
import oracle_lib as o
import rv32_link_programs as LP
import rv32_mem_programs as GP
import test_rv32_link as TL
import test_rv32_mem_chips as T
from raiko_amd import hal, p3, rv32, rv32elf, rv32link, rv32mem
from raiko_amd import executor as X
from raiko_amd.segment import P

DATA = LP.DATA
EXTS = {"sp1": None, "risc0": P - 11}
_relay = {}


def relay():
    """-> (elf, Execution, program image, preps, journals, memory image): executed once"""
    if not _relay:
        elf = LP.relay_program()
        ex = X.execute(elf, T.INPUT, segment_limit_po2=LP.PO2, record_trace=True)
        image = rv32elf.program_image(elf)
        _relay["v"] = (elf, ex, image, rv32mem.preps_of(image), [rv32link.journal_of(m) for m in ex.mem], rv32link.memory_image(elf))
    return _relay["v"]


def replayed_memory(elf, ex):
    """the guest's memory after the run by the plain-Python replay carried over its shards: {word address: word}"""
    memory, pos = None, 0
    for s, (_c, data), (start, _end, ecalls), _mem in T._shards(ex):
        _acc, memory, pos = GP.replay(elf, rv32.trace_of(s, data)[0], start, ecalls, T.INPUT, memory, pos)
    return memory


# ------------------------------------------------------------------------------------------------ the guest
def test_relay_is_the_run_the_file_states():
    elf, ex, _image, _preps, journals, mem_image = relay()
    assert len(ex.segments) == LP.N_SHARDS and all(s.po2 == LP.PO2 for s in ex.segments)
    assert tuple(s.cycles for s in ex.segments) == LP.CYCLES
    assert tuple(len(m) for m in ex.mem) == LP.ACCESSES
    assert tuple(len(j) for j in journals) == LP.JOURNAL_ROWS and journals[LP.EMPTY_SHARD].shape == (0, 3)
    assert tuple(rv32mem.memory_rows(m)[0].shape[0] for m in ex.mem) == LP.MEMORY_HEIGHTS
    # the chain against the replay
    final = rv32link.check_memory_chain(journals, mem_image)
    memory = replayed_memory(elf, ex)
    touched = {int(w) for m in ex.mem for w in m[:, 1]}
    assert set(final) == touched and len(touched) == LP.TOUCHED_WORDS
    assert final == {w: memory[w] for w in touched}
    assert final[(DATA + 12) >> 2] == LP.FINAL_AT_12 and final[(DATA + 4) >> 2] == 0xBEEF7FFF
    assert rv32link.check_memory_chain(journals, dict(zip(*[a.tolist() for a in mem_image]))) == final
    # the histories: the shards that touch each word, derived from the access lists
    shards_of = {}
    for k, m in enumerate(ex.mem):
        for w in sorted(set(m[:, 1].tolist())):
            shards_of.setdefault(w << 2, []).append(k)
    assert {a: tuple(v) for a, v in shards_of.items() if len(v) > 1} == LP.HISTORIES
    image = dict(zip(*[a.tolist() for a in mem_image]))
    assert image[(DATA + 4) >> 2] == LP.IMAGE_AT_4 and (DATA + 8) >> 2 in image and (DATA + 0x40) >> 2 not in image
    # what crosses each boundary: INIT in the later shard is FINAL in the earlier one, and no word of the image's
    row = lambda k, addr: journals[k][journals[k][:, 0] == addr >> 2][0].tolist()
    assert row(0, DATA + 8)[1:] == [GP.WORDS[2], LP.SEED_WORD] and row(3, DATA + 8)[1:] == [LP.SEED_WORD] * 2
    assert row(0, DATA + 0x40)[1:] == [0, T.INPUT[0]] and row(1, DATA + 0x40)[1:] == [T.INPUT[0]] * 2
    assert row(1, DATA + 0x48)[1:] == [0, T.INPUT[0]] and row(4, DATA + 0x48)[1:] == [T.INPUT[0]] * 2
    assert row(1, DATA + 0x104)[1:] == [0, LP.SEED_WORD] and row(4, DATA + 0x104)[1:] == [LP.SEED_WORD] * 2
    assert row(3, DATA + 4)[1:] == [LP.IMAGE_AT_4, 0xBEEF7FFF] and row(4, DATA + 4)[1:] == [0xBEEF7FFF] * 2


# ------------------------------------------------------------------------------------------------ the chain across gaps
def _with_init(journals, shard, addr, init):
    out = [j.copy() for j in journals]
    at = np.nonzero(out[shard][:, 0] == addr >> 2)[0]
    assert at.size == 1 and int(out[shard][at[0], 1]) != init
    out[shard][at[0], 1] = init
    return out


FORGERIES = {
    "gap, the image's word": (3, DATA + 8, GP.WORDS[2]),          # what a chain that forgot shard 0 would accept
    "gap, zero": (3, DATA + 8, 0),
    "gap, another word": (3, DATA + 8, 0x56781234),
    "gap over two, zero": (4, DATA + 0x48, 0),                    # outside the image: a chain that forgot shard 1 expects 0
    "gap over two, another word": (4, DATA + 0x48, T.INPUT[0] ^ 1),
    "late first touch, zero": (3, DATA + 4, 0),
    "late first touch, another word": (3, DATA + 4, LP.IMAGE_AT_4 ^ 0x10000),
    "late first touch, its later word": (3, DATA + 4, 0xBEEF7FFF),
    "ecall write, zero": (1, DATA + 0x40, 0),                     # the image's word instead of the ecall's
}


@pytest.mark.parametrize("name", sorted(FORGERIES))
def test_chain_refuses_a_forged_init_across_a_gap(name):
    _elf, _ex, _image, _preps, journals, mem_image = relay()
    shard, addr, init = FORGERIES[name]
    with pytest.raises(ValueError, match=r"shard %d: word 0x%08x " % (shard, addr)):
        rv32link.check_memory_chain(_with_init(journals, shard, addr, init), mem_image)


def test_image_word_of_the_gap_forgery_is_what_the_file_says():
    """the `gap, the image's word` forgery is the one a chain of neighbours accepts: it must really be the ELF's word"""
    _elf, _ex, _image, _preps, _journals, mem_image = relay()
    image = dict(zip(*[a.tolist() for a in mem_image]))
    assert image[(DATA + 8) >> 2] == GP.WORDS[2] != LP.SEED_WORD


def test_chain_does_not_place_an_empty_journal():
    """shard 2's journal is empty, so the chain check cannot tell whether it stands before or after shard 3's: the run
    with the two exchanged passes it, with the same final words.  The ORDER of an empty journal is bound by the digest
    in each shard's public values (tests/test_gpu_rv32_link_runs.py::test_relay_end_to_end holds that: the exchanged
    journals are refused at shard 2)"""
    _elf, _ex, _image, _preps, journals, mem_image = relay()
    swapped = [journals[0], journals[1], journals[3], journals[2], journals[4]]
    assert rv32link.check_memory_chain(swapped, mem_image) == rv32link.check_memory_chain(journals, mem_image)
    # any other exchange of neighbours is refused
    for k in (0, 1, 3):
        other = list(journals)
        other[k], other[k + 1] = other[k + 1], other[k]
        if k == 1:                                   # shards 1 and 2: the same run, the empty journal one place earlier
            assert rv32link.check_memory_chain(other, mem_image) == rv32link.check_memory_chain(journals, mem_image)
        else:
            with pytest.raises(ValueError, match="shard %d" % k):
                rv32link.check_memory_chain(other, mem_image)


# ------------------------------------------------------------------------------------------------ the other extension
@pytest.fixture(scope="module", params=sorted(EXTS))
def link_airs(request):
    return rv32link.airs(EXTS[request.param])


@pytest.mark.parametrize("k", range(LP.N_SHARDS))
def test_linked_airs_hold_on_every_relay_shard(link_airs, k):
    _elf, ex, image, preps, journals, _mem_image = relay()
    airs = link_airs
    assert [a.width for a in airs] == [a.width for a in rv32mem.airs()] and airs[8].n_public == rv32link.N_DIGEST
    s, (_c, data), (start, end, ecalls), mem = list(T._shards(ex))[k]
    canon, pc, pr, digest = rv32link.shard_tables(s, data, start, end, ecalls, image, mem)
    assert canon[8].shape[0] == LP.MEMORY_HEIGHTS[k]
    assert np.array_equal(rv32link.journal_of_table(canon[8]), journals[k])
    pubs = [pc, (), pr] + [()] * 5 + [p3.from_mont(digest)]
    assert T._check(airs, canon, preps, pubs, cpu_rows=s.cycles) == {}
    bal = rv32link.bus_balance(T._joined(canon, preps), airs)
    assert bal.pop(rv32link.BUS_LINK) == TL._stripped(rv32link.journal_tuples(journals[k]))
    assert all(v == {} for v in bal.values())
    if k == LP.EMPTY_SHARD:
        assert TL._stripped(rv32link.journal_tuples(journals[k])) == {} and not canon[8].any() and not canon[7][:, :rv32mem.G_ONE].any()
    assert np.array_equal(digest, rv32link.journal_root(journals[k], canon[8].shape[0].bit_length() - 1))


def test_unlinked_airs_hold_under_the_other_extension():
    _elf, ex, image, preps = T._run("ops")
    airs = rv32mem.airs(P - 11)
    assert [a.width for a in airs] == [a.width for a in rv32mem.airs()]
    s, (_c, data), (start, end, ecalls), mem = next(T._shards(ex))
    canon, pc, pr = rv32mem.shard_tables(s, data, start, end, ecalls, image, mem)
    assert T._check(airs, canon, preps, [pc, (), pr] + [()] * 6, cpu_rows=s.cycles) == {}
    assert all(v == {} for v in rv32mem.bus_balance(T._joined(canon, preps), airs).values())
    for a in airs:
        assert a.log_quotient_degree() <= 1
        a.handle()


# ------------------------------------------------------------------------------------------------ the digest under every set
DIGEST_SETS = dict(LP.LINK_SETS, risc0_field=(1, dict(LP.FAST, **PS.PARAM_SETS["risc0_field"][1])))
DIGEST_CASES = {"k0": (0, 1), "k3": (3, 2), "k62": (62, 6), "k300": (300, 9), "relay": None}


def _case_journals(case):
    """[(journal, log_rows)] of a case: a seeded journal of k rows, or relay's five at their own heights"""
    if DIGEST_CASES[case] is None:
        return [(j, h.bit_length() - 1) for j, h in zip(relay()[4], LP.MEMORY_HEIGHTS)]
    k, log_rows = DIGEST_CASES[case]
    return [(TL._journal(k, seed=7), log_rows)]


def _oracle_root(journal, log_rows):
    """or_mmcs_commit of the link matrix under the oracle's current parameters"""
    m = rv32link.link_matrix(journal, log_rows)
    mats = (o.OrMatrix * 1)()
    mats[0].values, mats[0].height, mats[0].width, mats[0].row_major = m.ctypes.data, m.shape[0], m.shape[1], 1
    nodes = np.zeros((2 * m.shape[0], 8), dtype=np.uint32)
    o.oracle().or_mmcs_commit(mats, 1, o.ptr(nodes))
    return nodes[1].copy()


@pytest.mark.parametrize("case", sorted(DIGEST_CASES))
@pytest.mark.parametrize("pset", sorted(DIGEST_SETS))
def test_journal_root_under_every_set_is_the_oracles(pset, case):
    preset, over = DIGEST_SETS[pset]
    blob = hal.make_params(preset, **over)
    o.oracle_set_params(preset, **over)
    try:
        for j, lg in _case_journals(case):
            assert np.array_equal(rv32link.journal_root(j, lg, blob), _oracle_root(j, lg)), (len(j), lg)
    finally:
        o.oracle_set_params()


@pytest.mark.parametrize("case", sorted(DIGEST_CASES))
def test_three_hashes_give_three_roots(case):
    """risc0_field changes the field's extension and the FRI parameters, not the hash: its roots are sp1's.  risc0 (a
    width-24 sponge) and m4_0_tables (another width-16 permutation) each give roots of their own -- also for an empty
    journal, where the digests of the all-zero subtrees already differ"""
    blobs = {name: hal.make_params(preset, **over) for name, (preset, over) in DIGEST_SETS.items()}
    for j, lg in _case_journals(case):
        roots = {name: rv32link.journal_root(j, lg, b).tobytes() for name, b in blobs.items()}
        assert roots["risc0_field"] == roots["sp1"] == rv32link.journal_root(j, lg).tobytes()
        assert len(set(roots.values())) == 3, (len(j), lg)
