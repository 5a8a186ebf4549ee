"""The link between shard memories on the CPU (raiko_amd/rv32link.py, rk_p3_verify_claims, rk_rv32mem_journal_root,
rk_exec_memory_image): claims in the host verifier against an exact-integer claim sum (tests/p3_ref_claims.py), the
linked memory AIR on the numpy tables of every guest, the journal's digest against the oracle's MMCS root, the ELF's
memory image against a byte array filled in header order, and the chain check on honest and forged runs -- the forged
second shard of tests/test_rv32_mem_chips.py::test_two_shards_chain_and_the_boundary_is_free among them, which is what
the link is for.  Every comparison is bit-exact."""
import struct
from collections import Counter

import numpy as np
import pytest

import oracle_lib as o
import p3_ref_claims as RC
import rv32_asm as A
import rv32_mem_programs as GP
import test_rv32_mem_chips as T
from raiko_amd import _lib, hal, p3, rv32, rv32link, rv32mem
from raiko_amd import executor as X
from raiko_amd.segment import P

FAST = dict(queries=8, pow_bits=6)
INIT = p3.to_mont([167009, 10])


@pytest.fixture(scope="module")
def blob():
    return hal.make_params(1, **FAST)


@pytest.fixture(scope="module")
def demo():
    """lookup_demo's four tables and the three without `add`, each proven by the oracle's prover (whose zero-sum check is
    in or_p3_verify only); the live cpu rows' (a, b, a + b), repeats included"""
    airs = p3.lookup_demo_airs()
    full = p3.lookup_demo_tables(5, airs=airs)
    three = [full[0], full[2], full[3]]
    o.oracle_set_params(1, **FAST)
    try:
        proof3, proof4 = o.oracle_p3_prove(three, INIT), o.oracle_p3_prove(full, INIT)
    finally:
        o.oracle_set_params()
    cpu = p3.from_mont(full[0].trace).astype(np.int64)
    live = cpu[cpu[:, 4] == 1][:, :3]
    assert len(live) > len(np.unique(live, axis=0))             # repeats: every tuple still counts once per row
    return full, three, proof3, proof4, live


def _claim(live, bus=p3.BUS_ADD, sign=-1):
    return [(bus, sign, p3.to_mont(live))]


def test_claims_replace_the_missing_table(demo, blob):
    full, three, proof3, proof4, live = demo
    assert p3.verify(three, proof3, INIT, blob) == 8
    assert p3.verify(three, proof3, INIT, blob, claims=_claim(live)) == 0
    altered, added = live.copy(), np.concatenate([live, live[:1]])
    altered[3, 2] = (altered[3, 2] + 1) % P
    cases = {"honest": _claim(live), "altered": _claim(altered), "dropped": _claim(live[1:]), "added": _claim(added),
             "sign": _claim(live, sign=1), "bus": _claim(live, bus=p3.BUS_MUL), "none": [],
             "split": _claim(live[:5]) + _claim(live[5:])}
    for name, claims in cases.items():
        got = p3.verify(three, proof3, INIT, blob, claims=claims)
        assert got == (0 if name in ("honest", "split") else 8), name
        # the accept / reject boundary against the claim sum in exact integers
        ref = [(b, s, p3.from_mont(t).astype(np.int64).tolist()) for b, s, t in claims]
        assert RC.accepts(1, three, INIT, proof3, ref) == (got == 0), name
    # no claims: rk_p3_verify's verdicts, on the untouched four-table proof and on damaged ones
    assert p3.verify(full, proof4, INIT, blob, claims=[]) == p3.verify(full, proof4, INIT, blob) == 0
    for at in (0, 12, proof4.size - 1):
        bad = proof4.copy()
        bad[at] = (int(bad[at]) + 1) % P
        assert p3.verify(full, bad, INIT, blob, claims=[]) == p3.verify(full, bad, INIT, blob) != 0
    assert p3.verify(full, proof4[:-1], INIT, blob, claims=[]) == p3.verify(full, proof4[:-1], INIT, blob) == 1
    # the four tables balance on their own: a claim on top unbalances them
    assert p3.verify(full, proof4, INIT, blob, claims=_claim(live[:1])) == 8


def test_malformed_claims_are_invalid(demo, blob):
    _full, three, proof3, _proof4, live = demo
    inv = _lib.RK_ERR_INVALID
    long_ = np.concatenate([live, live[:, :1]], axis=1)          # four values: the tables' challenges cover three
    assert p3.verify(three, proof3, INIT, blob, claims=_claim(long_)) == inv
    words = p3.to_mont(live)
    words[2, 1] = P                                              # not a canonical word
    assert p3.verify(three, proof3, INIT, blob, claims=[(p3.BUS_ADD, -1, words)]) == inv
    for sign in (0, 2, -2):
        assert p3.verify(three, proof3, INIT, blob, claims=_claim(live, sign=sign)) == inv
    # claims against tables without lookups
    fib = [p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(4))]
    o.oracle_set_params(1, **FAST)
    try:
        pf = o.oracle_p3_prove(fib, INIT)
    finally:
        o.oracle_set_params()
    assert p3.verify(fib, pf, INIT, blob) == p3.verify(fib, pf, INIT, blob, claims=[]) == 0
    assert p3.verify(fib, pf, INIT, blob, claims=[(1, -1, p3.to_mont(np.array([[1]])))]) == inv
    # a short tuple is read as padded with zeros, as an interaction's
    short = p3.to_mont(np.array([[5, 0, 0]])), p3.to_mont(np.array([[5]]))
    a, b = (RC.claim_total(1, three, INIT, proof3, [(p3.BUS_ADD, -1, p3.from_mont(t).astype(np.int64).tolist())]) for t in short)
    assert a == b


# ------------------------------------------------------------------------------------------------ the linked AIR
RUNS = dict(GP.GUESTS, two=GP.two_shard_program, count0=lambda: GP.count_program(0), count1=lambda: GP.count_program(1),
            count129=lambda: GP.count_program(129))
_runs = {}


def _run(name):
    if name not in _runs:
        elf = RUNS[name]()
        ex = X.execute(elf, T.INPUT, segment_limit_po2=13, record_trace=True)
        image = rv32mem.rv32elf.program_image(elf)
        _runs[name] = (elf, ex, image, rv32mem.preps_of(image))
    return _runs[name]


@pytest.fixture(scope="module")
def airs():
    return rv32link.airs()


def _stripped(tuples):
    """bus_balance's reading of a tuple: trailing zeros dropped"""
    out = Counter()
    for t in tuples.tolist():
        while t and t[-1] == 0:
            t.pop()
        out[tuple(t)] += 1
    return dict(out)


@pytest.mark.parametrize("name", sorted(RUNS))
def test_linked_air_holds_and_leaves_the_journal_on_the_link_bus(name, airs):
    _elf, ex, image, preps = _run(name)
    assert [a.width for a in airs] == [a.width for a in rv32mem.airs()] and airs[8].n_public == 8
    assert [a.prep_width for a in airs] == [a.prep_width for a in rv32mem.airs()]
    assert airs[8].log_quotient_degree() <= 1
    airs[8].handle()
    for k, (s, (_c, data), (start, end, ecalls), mem) in enumerate(T._shards(ex)):
        canon, pc, pr, digest = rv32link.shard_tables(s, data, start, end, ecalls, image, mem)
        journal = rv32link.journal_of(mem)
        assert np.array_equal(journal, rv32link.journal_of_table(canon[8]))
        assert (np.diff(journal[:, 0].astype(np.int64)) > 0).all() and len(journal) == np.unique(mem[:, 1]).size
        pubs = [pc, (), pr] + [()] * 5 + [p3.from_mont(digest)]
        assert T._check(airs, canon, preps, pubs, cpu_rows=s.cycles) == {}
        bal = rv32link.bus_balance(T._joined(canon, preps), airs)
        assert bal.pop(rv32link.BUS_LINK) == _stripped(rv32link.journal_tuples(journal)), (name, k)
        assert all(v == {} for v in bal.values())
        assert np.array_equal(digest, rv32link.journal_root(journal, canon[8].shape[0].bit_length() - 1))
    if name == "count0":
        assert len(journal) == 0 and canon[8].shape[0] == 2
    if name == "count129":
        assert len(journal) == 1


@pytest.mark.parametrize("ext", ["sp1", "risc0"])
def test_forged_boundary_rows_under_the_linked_air(airs, ext):
    """the forgeries of test_rv32_mem_chips.py::test_forged_boundary_rows, refused by the same named constraints, with
    the AIRs built for either extension (x^4 - 3, x^4 + 11)"""
    airs = airs if ext == "sp1" else rv32link.airs(P - 11)
    _elf, ex, image, preps = T._run("forge")
    s, (_c, data), (start, end, ecalls), mem = next(T._shards(ex))
    canon = rv32link.shard_tables(s, data, start, end, ecalls, image, mem)[0]
    B, air = rv32mem, airs[8]
    pub = [0] * 8
    base = canon[8]
    real = int(base[:, B.B_REAL].sum())
    assert real >= 3 and air.check_trace(base, pub) == []
    assert air.constraint_names == rv32mem.memory_air().constraint_names
    bus = lambda t: rv32link.bus_balance(T._joined(canon[:8] + [t], preps), airs)
    for same in (0, 1):
        t = base.copy()
        t[1] = t[0]
        t[0, B.B_SAME], t[0, B.B_GL], t[0, B.B_GH] = same, 0, 0
        assert (0, "ascending low" if same else "ascending high") in T._named(air, air.check_trace(t, pub))
        t[0, B.B_GL if same else B.B_GH] = P - 1
        assert not any(r == 0 for r, _k in air.check_trace(t, pub)) and bus(t)[rv32.BUS_RANGE16]
    t = base.copy()
    t[[0, 1]] = t[[1, 0]]
    assert {k for r, k in T._named(air, air.check_trace(t, pub)) if r == 0} & {"ascending low", "ascending high", "same high"}
    t = base.copy()
    t[real - 2] = 0
    assert (real - 2, "padding") in T._named(air, air.check_trace(t, pub))


# ------------------------------------------------------------------------------------------------ the digest
def _journal(k, seed=0):
    g = np.random.default_rng(seed + k)
    addr = np.sort(g.choice(1 << 30, size=k, replace=False)).astype(np.uint32)
    return np.stack([addr, g.integers(0, 1 << 32, size=k).astype(np.uint32), g.integers(0, 1 << 32, size=k).astype(np.uint32)], axis=1)


def _oracle_root(journal, log_rows):
    m = rv32link.link_matrix(journal, log_rows)
    mats = (o.OrMatrix * 1)()
    mats[0].values, mats[0].height, mats[0].width, mats[0].row_major = m.ctypes.data, m.shape[0], m.shape[1], 1
    nodes = np.zeros((2 * m.shape[0], 8), dtype=np.uint32)
    o.oracle_set_params(1)
    try:
        o.oracle().or_mmcs_commit(mats, 1, o.ptr(nodes))
    finally:
        o.oracle_set_params()
    return nodes[1].copy()


@pytest.mark.parametrize("k, log_rows", [(0, 1), (1, 1), (2, 1), (0, 2), (1, 2), (2, 2), (3, 2), (4, 2), (300, 9), (512, 9)])
def test_journal_root_is_the_mmcs_root_of_the_link_matrix(k, log_rows):
    j = _journal(k)
    if k:
        j[0, 0], j[-1, 0] = (0 if k > 1 else 5), (1 << 30) - 1              # the address range's ends
        j[0, 1:] = 0xFFFFFFFF
    got = rv32link.journal_root(j, log_rows)
    assert np.array_equal(got, _oracle_root(j, log_rows))
    assert np.array_equal(got, rv32link.journal_root(j, log_rows, hal.make_params(1, **FAST)))   # the query count is no part of it
    if k:
        other = j.copy()
        other[k // 2, 2] ^= 1
        assert not np.array_equal(got, rv32link.journal_root(other, log_rows))


def test_journal_root_refuses_malformed_journals():
    j = _journal(3)
    for bad, log_rows in ((j, 1), (j[[0, 2, 1]], 2), (j[[0, 0, 1]], 2), (j, 0)):
        with pytest.raises(_lib.RkError):
            rv32link.journal_root(bad, log_rows)
    high = j.copy()
    high[2, 0] = 1 << 30
    with pytest.raises(_lib.RkError):
        rv32link.journal_root(high, 2)


# ------------------------------------------------------------------------------------------------ the memory image
def _make_elf(segments):
    """segments: [(vaddr, file bytes, memsz)] as PT_LOAD headers in that order"""
    n = len(segments)
    off = 52 + 32 * n
    head = b"\x7fELF" + bytes([1, 1, 1]) + bytes(9) + struct.pack("<HHIIIIIHHHHHH", 2, 243, 1, 0x1000, 52, 0, 0, 52, 32, n, 40, 0, 0)
    ph, body = b"", b""
    for vaddr, data, memsz in segments:
        ph += struct.pack("<IIIIIIII", 1, off + len(body), vaddr, vaddr, len(data), memsz, 6, 4)
        body += data
    return head + ph + body


def _image_restated(elf):
    """a byte array filled in program-header order -> {word address: word} over the words that hold a file byte"""
    mem, seen = {}, set()
    phoff, = struct.unpack_from("<I", elf, 28)
    phentsize, phnum = struct.unpack_from("<HH", elf, 42)
    for i in range(phnum):
        p_type, off, vaddr, _pa, filesz, _memsz, _fl = struct.unpack_from("<IIIIIII", elf, phoff + i * phentsize)
        if p_type == 1:
            for b in range(filesz):
                mem[vaddr + b] = elf[off + b]
                seen.add((vaddr + b) >> 2)
    return {w: sum(mem.get(4 * w + k, 0) << (8 * k) for k in range(4)) for w in sorted(seen)}


HAND = {
    "overlap": [(0x1000, bytes(range(1, 17)), 16), (0x1008, b"\xaa\xbb\xcc\xdd\xee\xff\x11\x22\x33\x44\x55\x66", 12)],
    "unaligned": [(0x2001, b"\x10\x20\x30\x40\x50\x60", 6)],
    "bss": [(0x3000, b"\x01\x02\x03\x04\x05", 64)],
    "later first": [(0x5002, b"\x99\x98", 2), (0x5000, b"\x01\x02\x03", 3), (0x4ffc, b"\x07", 1)],
    "empty": [(0x6000, b"", 16)],
}


@pytest.mark.parametrize("name", sorted(HAND) + sorted(RUNS))
def test_memory_image_is_the_loaders(name):
    elf = _make_elf(HAND[name]) if name in HAND else RUNS[name]()
    addr, words = rv32link.memory_image(elf)
    want = _image_restated(elf)
    assert dict(zip(addr.tolist(), words.tolist())) == want and addr.tolist() == sorted(want)
    if name == "overlap":
        assert want[0x1008 >> 2] == 0xDDCCBBAA and want[0x1004 >> 2] == 0x08070605
    if name == "unaligned":
        assert want == {0x2000 >> 2: 0x30201000, 0x2004 >> 2: 0x00605040}
    if name == "bss":
        assert want == {0x3000 >> 2: 0x04030201, 0x3004 >> 2: 5}
    if name == "later first":
        assert want == {0x4ffc >> 2: 7, 0x5000 >> 2: 0x98030201}
    if name == "empty":
        assert addr.size == 0
    # the capacity protocol: the count without buffers, RK_ERR_CAPACITY one short, the words at exactly enough
    import ctypes as C
    lib, n = _lib.load(), C.c_size_t(77)
    up = lambda arr: arr.ctypes.data_as(_lib.u32p)
    st = lib.rk_exec_memory_image(elf, len(elf), None, None, 0, C.byref(n))
    assert n.value == len(want) and st == (_lib.RK_ERR_CAPACITY if want else 0)
    if want:
        a, w = np.full(len(want), 0xDEADBEEF, dtype=np.uint32), np.full(len(want), 0xDEADBEEF, dtype=np.uint32)
        assert lib.rk_exec_memory_image(elf, len(elf), up(a), up(w), len(want) - 1, C.byref(n)) == _lib.RK_ERR_CAPACITY
        assert n.value == len(want) and (a == 0xDEADBEEF).all()
        assert lib.rk_exec_memory_image(elf, len(elf), up(a), up(w), len(want), C.byref(n)) == 0 and a.tolist() == sorted(want)
    assert lib.rk_exec_memory_image(elf[:40], 40, None, None, 0, C.byref(n)) == _lib.RK_ERR_INVALID


def test_memory_image_is_what_the_executor_loads():
    """the guests' first accesses read the image's words"""
    elf, ex, _image, _preps = _run("ops")
    image = dict(zip(*[a.tolist() for a in rv32link.memory_image(elf)]))
    assert [image[(GP.DATA >> 2) + k] for k in range(4)] == list(GP.WORDS)
    first = {}
    for _c, w, before, _after in ex.mem[0].tolist():
        first.setdefault(w, before)
    assert all(image.get(w, 0) == v for w, v in first.items())


# ------------------------------------------------------------------------------------------------ the chain
def _two():
    elf, ex, _image, _preps = _run("two")
    return elf, ex, [rv32link.journal_of(m) for m in ex.mem], rv32link.memory_image(elf)


def forged_second_shard(ex):
    """the second shard of `two` as test_two_shards_chain_and_the_boundary_is_free forges it: the word the first shard
    left at 0x5EEDBEEF starts from 0x56781234, and the load returns that -> (data, mem) of the forged shard"""
    s, (_c, data), (_start, _end, _ecalls), mem = list(T._shards(ex))[1]
    tr = rv32.trace_of(s, data)[0]
    c = tr["ins"].tolist().index(A.encode("lw", ("a2", 8, "s0"), 0, {}))
    data, mem = data.copy(), mem.copy()
    data[rv32.RES_LO, c], data[rv32.RES_HI, c] = p3.to_mont([0x1234, 0x5678])
    k = np.nonzero(mem[:, 0] == c)[0][0]
    mem[k, 2] = mem[k, 3] = 0x56781234
    return data, mem


def test_chain_of_the_honest_run_returns_the_executors_words():
    elf, ex, journals, image = _two()
    final = rv32link.check_memory_chain(journals, image)
    memory, pos = None, 0
    for s, (_c, data), (start, _end, ecalls), _mem in T._shards(ex):
        _acc, memory, pos = GP.replay(elf, rv32.trace_of(s, data)[0], start, ecalls, T.INPUT, memory, pos)
    assert final == {w: memory[w] for w in final} and set(final) == {int(w) for m in ex.mem for w in m[:, 1]}
    assert final[(GP.DATA + 8) >> 2] == 0x5EEDBEEF
    assert rv32link.check_memory_chain(journals, dict(zip(*[a.tolist() for a in image]))) == final
    # every guest's single shard starts from the image
    for name in sorted(GP.GUESTS):
        g_elf, g_ex, _i, _p = _run(name)
        rv32link.check_memory_chain([rv32link.journal_of(m) for m in g_ex.mem], rv32link.memory_image(g_elf))


def test_chain_refuses_forged_boundaries():
    _elf, ex, journals, image = _two()
    w = (GP.DATA + 8) >> 2
    # the forged second shard: per shard nothing is wrong (test_rv32_mem_chips.py), the chain names it
    _data, mem = forged_second_shard(ex)
    forged = rv32link.journal_of(mem)
    assert forged[forged[:, 0] == w][0, 1] == 0x56781234
    with pytest.raises(ValueError, match=r"shard 1: word 0x%08x" % (w << 2)):
        rv32link.check_memory_chain([journals[0], forged], image)
    # a first shard whose INIT is not the ELF's data word
    j0 = journals[0].copy()
    row = int(np.nonzero(j0[:, 0] == GP.DATA >> 2)[0][0])
    assert j0[row, 1] == GP.WORDS[0]
    j0[row, 1] ^= 0x100
    with pytest.raises(ValueError, match=r"shard 0: word 0x%08x" % GP.DATA):
        rv32link.check_memory_chain([j0, journals[1]], image)
    # a word outside the image starts from non-zero
    far = np.array([[(GP.DATA + 0x4000) >> 2, 1, 1]], dtype=np.uint32)
    assert rv32link.check_memory_chain([far * [1, 0, 1]], image) == {int(far[0, 0]): 1}
    with pytest.raises(ValueError, match=r"shard 0: word 0x%08x" % (GP.DATA + 0x4000)):
        rv32link.check_memory_chain([far], image)
    # the journals of the two shards swapped
    with pytest.raises(ValueError, match="shard 0"):
        rv32link.check_memory_chain(journals[::-1], image)


def test_link_is_a_keyword_of_the_rv32im_mem_set_only():
    assert X.CHIPS == ("trace",) + X.RV32_CHIPS and X.KEYED_CHIPS == ("rv32im-elf", "rv32im-mem")
    from raiko_amd import p3_exec, rv32_sets
    for chips in ("rv32i", "rv32im-elf", "trace"):
        with pytest.raises(ValueError):
            p3_exec.execute_and_prove_p3(b"", chips=chips, link=True)
        with pytest.raises(ValueError):
            p3_exec.P3Pipeline(chips=chips, link=True)
    with pytest.raises(ValueError):
        rv32_sets._rv32_airs_of("rv32im", link=True)
    assert [a.width for a in rv32_sets._rv32_airs_of("rv32im-mem", link=True)] == [a.width for a in rv32link.airs()]
    # the numpy shards: rv32mem's tables, the memory table's public values the digest, the journal beside them
    _elf, ex, image, _preps = _run("two")
    plain = rv32_sets.shards("rv32im-mem", ex, image)
    linked = rv32_sets.shards("rv32im-mem", ex, image, link=True)
    for (pt, pi), (lt, li, journal), mem in zip(plain, linked, ex.mem):
        assert all(np.array_equal(a.trace, b.trace) for a, b in zip(pt, lt)) and np.array_equal(pi, li)
        assert np.array_equal(journal, rv32link.journal_of(mem))
        assert np.array_equal(lt[8].public_values, rv32link.journal_root(journal, lt[8].log_height)) and pt[8].public_values.size == 0
