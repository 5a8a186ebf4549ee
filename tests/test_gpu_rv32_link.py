"""The link between shard memories on the GPU: rk_rv32mem_journal_device (mem_journal_kernel and the library's commitment
of the link matrix) against numpy word for word; link=False unchanged; the two-shard guest end to end through the shard
pool and through the pipeline; the forged second shard of tests/test_rv32_link.py -- whose shard proof verifies -- refused
by the chain check, where the same run without the link verifies; and the pool's verifiers refusing altered claims.

mem_journal_kernel runs one block of min(rows, 128) lanes per 128 table rows.  Sizes where it takes another path: 2 rows
(a block of two lanes, less than a wave); 128 rows (the tallest table of one block); 256 rows (the first with a second
block, whose lane 0 reads REAL of the row before its tile from HBM, not from LDS); 512 rows (`distinct`: 300 words).
Every case runs at po2 = 13 with 8 queries; every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import rv32_mem_programs as GP
from test_rv32_link import forged_second_shard
from raiko_amd import _lib, p3, rv32, rv32elf, rv32link, rv32mem, rv32_sets
from raiko_amd import executor as X
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

INPUT = [0x11223344, 0x80FF7F01, 0xDEADBEEF, 0x00000044]
FAST = dict(queries=8, pow_bits=6)
SHAPES = {"count0": lambda: GP.count_program(0), "count1": lambda: GP.count_program(1), "count129": lambda: GP.count_program(129),
          "distinct": lambda: GP.count_program(300, distinct=True), "two": GP.two_shard_program,
          "rows128": lambda: GP.count_program(128, distinct=True), "rows256": lambda: GP.count_program(129, distinct=True)}
ROWS = {"count0": [2], "count1": [2], "count129": [2], "distinct": [512], "two": [2, 4], "rows128": [128], "rows256": [256]}


@pytest.fixture(scope="module")
def hal():
    h = H.HipHal(0)
    h.set_params(1, **FAST)
    yield h
    h.close()


@pytest.fixture(scope="module")
def blob():
    return H.make_params(1, **FAST)


def _memory_tables(name):
    """the canonical memory table of every shard of a guest (numpy)"""
    ex = X.execute(SHAPES[name](), INPUT, segment_limit_po2=13, record_trace=True)
    return [rv32mem.memory_rows(m)[0] for m in ex.mem]


def _on_device(hal, table):
    buf = hal.copy_from_elem(np.ascontiguousarray(p3.to_mont(table)).reshape(-1))
    hal.sync()
    return buf


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_journal_device_equals_numpy(hal, blob, name):
    tables = _memory_tables(name)
    assert [t.shape[0] for t in tables] == ROWS[name]
    for t in tables:
        lg = t.shape[0].bit_length() - 1
        want = rv32link.journal_of_table(t)
        buf = _on_device(hal, t)
        try:
            root, journal, link, n_real = rv32_sets.journal_device(hal, buf, lg, keep=True)
        finally:
            buf.free()
        assert n_real == len(want) == int(t[:, rv32mem.B_REAL].sum())
        assert np.array_equal(journal, want)
        assert np.array_equal(link, rv32link.link_matrix(want, lg))
        assert np.array_equal(root, rv32link.journal_root(want, lg, blob))
    # a table taller than its words need: the digest is the taller table's
    t = np.concatenate([tables[0], np.zeros_like(tables[0])])
    buf = _on_device(hal, t)
    try:
        root, journal = rv32_sets.journal_device(hal, buf, t.shape[0].bit_length() - 1)
    finally:
        buf.free()
    assert np.array_equal(journal, rv32link.journal_of_table(tables[0]))
    assert np.array_equal(root, rv32link.journal_root(journal, t.shape[0].bit_length() - 1, blob))


def test_journal_device_refuses_a_malformed_table(hal):
    """REAL 1 after a 0 (inside a block and across the block boundary at row 128), REAL = 2, a limb of 2^16, WL = 2^14:
    RK_ERR_INVALID, nothing is handed back"""
    base = _memory_tables("rows256")[0]
    assert base.shape[0] == 256 and int(base[:, rv32mem.B_REAL].sum()) == 129
    bad = []
    for row in (5, 127):                                       # 127: row 128 is the first of the second block
        t = base.copy()
        t[row] = 0
        bad.append(t)
    for col, v in ((rv32mem.B_REAL, 2), (rv32mem.B_F_HI, 1 << 16), (rv32mem.B_I_LO, 1 << 16), (rv32mem.B_WH, 1 << 16), (rv32mem.B_WL, 1 << 14)):
        t = base.copy()
        t[128 if col == rv32mem.B_WH else 3, col] = v
        bad.append(t)
    for t in bad:
        buf = _on_device(hal, t)
        try:
            with pytest.raises(_lib.RkError) as e:
                rv32_sets.journal_device(hal, buf, 8)
            assert e.value.status == _lib.RK_ERR_INVALID
        finally:
            buf.free()
    t = base.copy()                                            # a limb out of range on a padding row is nobody's
    t[200, rv32mem.B_GL] = 1 << 20
    buf = _on_device(hal, t)
    try:
        assert np.array_equal(rv32_sets.journal_device(hal, buf, 8)[1], rv32link.journal_of_table(base))
    finally:
        buf.free()


def test_journal_device_refuses_wrong_sizes_before_launch(hal):
    lib = _lib.load()
    rows = 8
    bufs = [hal.alloc_elem(n * rows) for n in (13, 3, 6, 16)]
    try:
        for b in bufs:
            b.copy_from(np.full(b.words, 7, dtype=np.uint32))
        mem, journal, link, nodes = [C.c_void_p(b.ptr) for b in bufs]
        root, n = np.zeros(8, dtype=np.uint32), C.c_size_t(0)
        r = root.ctypes.data_as(_lib.u32p)
        call = lambda m, rws, j, lk, nd, cnt, rt: lib.rk_rv32mem_journal_device(hal._ctx, m, rws, j, lk, nd, cnt, rt)
        for rws in (0, 1, 3, 6, 12):
            assert call(mem, rws, journal, link, nodes, C.byref(n), r) == _lib.RK_ERR_INVALID
        assert call(None, rows, journal, link, nodes, C.byref(n), r) == _lib.RK_ERR_INVALID
        assert call(mem, rows, None, link, nodes, C.byref(n), r) == _lib.RK_ERR_INVALID
        assert call(mem, rows, journal, None, nodes, C.byref(n), r) == _lib.RK_ERR_INVALID
        assert call(mem, rows, journal, link, None, C.byref(n), r) == _lib.RK_ERR_INVALID
        assert call(mem, rows, journal, link, nodes, None, r) == _lib.RK_ERR_INVALID
        assert call(mem, rows, journal, link, nodes, C.byref(n), None) == _lib.RK_ERR_INVALID
        hal.sync()
        assert all((b.to_host() == 7).all() for b in bufs) and not root.any()
    finally:
        for b in bufs:
            b.free()


def _free(bufs):
    for d in bufs:
        for b, _lg in d:
            b.free()


def test_link_false_is_unchanged_and_the_key_is_shared(hal, blob):
    elf = GP.two_shard_program()
    plain = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem")
    try:
        linked = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", link=True)
        try:
            assert np.array_equal(plain.root, linked.root) and plain.program_log_height == linked.program_log_height
            assert [a.n_public for a in plain.airs] == [4, 0, 128, 0, 0, 0, 0, 0, 0] and linked.airs[8].n_public == 8
            out = X.execute_rv32_device(hal, elf, INPUT, 13, chips="rv32im-mem", key=plain)
            assert len(out) == 4
            _ex, shards, _dev, bufs = out
            try:
                lout = X.execute_rv32_device(hal, elf, INPUT, 13, chips="rv32im-mem", key=linked, link=True)
                assert len(lout) == 5
                _lex, lshards, _ldev, lbufs, journals = lout
                try:
                    hal.sync()
                    ref_ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
                    ref = X.p3_rv32mem_shards(ref_ex, rv32elf.program_image(elf), airs=plain.airs)
                    for (rt, rinit), d, ld, (tables, init), (ltables, linit), j, mem in zip(ref, bufs, lbufs, shards, lshards, journals, ref_ex.mem):
                        assert len(tables) == len(ltables) == 9 and np.array_equal(init, rinit) and np.array_equal(linit, rinit)
                        assert tables[8].public_values.size == 0
                        for r, (b, lg), (lb, llg), t, lt in zip(rt, d, ld, tables, ltables):
                            got = b.to_host()
                            assert lg == llg and np.array_equal(got, r.trace.reshape(-1)) and np.array_equal(got, lb.to_host())
                        assert all(np.array_equal(t.public_values, lt.public_values) for t, lt in zip(tables[:8], ltables[:8]))
                        assert np.array_equal(j, rv32link.journal_of(mem))
                        assert np.array_equal(ltables[8].public_values, rv32link.journal_root(j, ltables[8].log_height, blob))
                finally:
                    _free(lbufs)
            finally:
                _free(bufs)
        finally:
            linked.close()
    finally:
        plain.close()


def _final_words(elf):
    """the executor's final words of everything the run touched, by the plain-Python replay of the guest"""
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    memory, pos = None, 0
    for s, (_c, data), (start, _end, ecalls) in zip(ex.segments, ex.witness, ex.rv32):
        _acc, memory, pos = GP.replay(elf, rv32.trace_of(s, data)[0], start, ecalls, INPUT, memory, pos)
    return ex, {int(w): memory[int(w)] for m in ex.mem for w in m[:, 1]}


def test_two_shards_end_to_end(blob):
    elf = GP.two_shard_program()
    ref_ex, final = _final_words(elf)
    want = [rv32link.journal_of(m) for m in ref_ex.mem]
    ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=13, params=blob, batch=2, chips="rv32im-mem", link=True)
    ex2, pproofs, _kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=13, params=blob, chips="rv32im-mem", link=True)
    assert len(proofs) == len(pproofs) == 2 and all(np.array_equal(a, b) for a, b in zip(proofs, pproofs))
    for e in (ex, ex2):
        assert len(e.journals) == 2 and all(np.array_equal(a, b) for a, b in zip(e.journals, want))
        assert e.final_memory == final and final[(GP.DATA + 8) >> 2] == 0x5EEDBEEF
    vk = dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height)
    image = rv32link.memory_image(elf)
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc, **vk, journals=ex.journals, image=image)
    for k, ((tables, init), pf) in enumerate(zip(shards, proofs)):
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=ex.journals[k]) == 0
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk) == 8               # nobody receives the journal
        assert p3.verify(X.rv32_verifier_tables(tables, pf, **vk), pf, init, blob, prep_root=ex.prep_root) == 8
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=ex.journals[1 - k]) != 0
        # its own journal, a digest word changed in the statement
        pv = tables[8].public_values.copy()
        pv[3] = (int(pv[3]) + 1) % rv32mem.P
        other = list(tables[:8]) + [p3.Table.pinned(tables[8].air, tables[8].log_height, pv)]
        assert X.verify_rv32_shard(other, pf, init, blob, **vk, journal=ex.journals[k]) == 2
        # a journal row altered: the digest no longer matches; with the digest bypassed the claims do not cancel
        j = ex.journals[k].copy()
        j[0, 2] ^= 1
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=j) == 2
        vt = X.rv32_verifier_tables(tables, pf, **vk)
        assert p3.verify(vt, pf, init, blob, prep_root=ex.prep_root, claims=rv32link.claims_of(j)) == 8
    with pytest.raises(ValueError, match="shard 0"):
        X.verify_rv32_execution(shards, proofs, blob, **vk, journals=ex.journals[::-1], image=image)


def _host_shard(airs, canon, pubs, preps, init):
    return [p3.Table(a, p3.to_mont(t), pv, prep=pm) for a, t, pv, pm in zip(airs, canon, pubs, preps)], init


def test_forged_second_shard_verifies_alone_and_the_chain_refuses_it(hal, blob):
    """the forgery the link is for: shard 1 starts the word shard 0 left at 0x5EEDBEEF from 0x56781234 and loads that.
    With the forger's own honest digest of its forged journal the shard proof verifies with its claims; the chain check
    refuses the run at shard 1.  Without the link the same run verifies"""
    elf = GP.two_shard_program()
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    image = rv32elf.program_image(elf)
    data, mem = forged_second_shard(ex)
    s, (start, _end, ecalls) = ex.segments[1], ex.rv32[1]
    for link in (True, False):
        key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", link=link)
        try:
            vk = dict(prep_root=key.root.copy(), program_log_height=key.program_log_height)
            preps = key.host_preps()
            honest = rv32_sets.shards("rv32im-mem", ex, image, airs=key.airs, link=link, params=blob)
            module = rv32link if link else rv32mem
            canon, pc, pr, *digest = module.shard_tables(s, data, start, None, ecalls, image, mem, **(dict(params=blob) if link else {}))
            pubs = [p3.to_mont(pc), (), p3.to_mont(pr)] + [()] * 5 + [digest[0] if link else ()]
            forged = _host_shard(key.airs, canon, pubs, preps, s.init_words())
            shards = [honest[0][:2], forged]
            journals = [honest[0][2], rv32link.journal_of(mem)] if link else None
            proofs = [p3.prove(hal, tables, init, key=key.key) for tables, init in shards]
            entry = ex.segments[0].start_pc
            if not link:
                assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=entry, **vk)
                continue
            for (tables, init), pf, j in zip(shards, proofs, journals):
                assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=j) == 0
            w = (GP.DATA + 8) >> 2
            with pytest.raises(ValueError, match=r"shard 1: word 0x%08x" % (w << 2)):
                X.verify_rv32_execution(shards, proofs, blob, entry_pc=entry, **vk, journals=journals, image=rv32link.memory_image(elf))
            # the honest run through the same route verifies
            hp = [proofs[0], p3.prove(hal, honest[1][0], honest[1][1], key=key.key)]
            assert X.verify_rv32_execution([h[:2] for h in honest], hp, blob, entry_pc=entry, **vk, journals=[h[2] for h in honest],
                                           image=rv32link.memory_image(elf))
        finally:
            key.close()


def test_pool_verifies_with_claims(hal, blob):
    elf = GP.two_shard_program()
    ex = X.execute(elf, INPUT, segment_limit_po2=13, record_trace=True)
    key = X.setup_rv32_elf(hal, elf, blob, chips="rv32im-mem", link=True)
    try:
        linked = rv32_sets.shards("rv32im-mem", ex, rv32elf.program_image(elf), airs=key.airs, link=True, params=blob)
        shards, journals = [h[:2] for h in linked], [h[2] for h in linked]
        claims = [rv32link.claims_of(j) for j in journals]
        proofs = p3.prove_shards(shards, blob, batch=2, verify=True, key=key.key, claims=claims)
        vk = dict(prep_root=key.root, program_log_height=key.program_log_height)
        for (tables, init), pf, j in zip(shards, proofs, journals):
            assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=j) == 0
        # without claims the pool's verifiers refuse the first shard they check; with one tuple altered, that shard
        with pytest.raises(_lib.RkError) as e:
            p3.prove_shards(shards, blob, batch=2, verify=True, key=key.key)
        assert e.value.status == _lib.RK_ERR_VERIFY and e.value.segment in (0, 1)
        bus, sign, tuples = claims[1][0]
        tuples = tuples.copy()
        tuples[0, 4] = p3.to_mont([(int(p3.from_mont(tuples[0, 4:5])[0]) + 1) % rv32mem.P])[0]
        with pytest.raises(_lib.RkError) as e:
            p3.prove_shards(shards, blob, batch=2, verify=True, key=key.key, claims=[claims[0], [(bus, sign, tuples)]])
        assert e.value.status == _lib.RK_ERR_VERIFY and e.value.segment == 1
        # verify = 0: nothing is checked
        assert len(p3.prove_shards(shards, blob, batch=2, verify=False, key=key.key, claims=[claims[0], [(bus, sign, tuples)]])) == 2
    finally:
        key.close()
