"""Linked rv32im-mem runs over many shards and under other parameter sets, on the GPU: the `relay` guest of
tests/rv32_link_programs.py -- five shards at po2 = 13, memory tables of 4, 64, 2, 2 and 4 rows, the third shard with an
empty journal -- and the sets of LINK_SETS (SP1's preset; risc0's, whose digest is a width-24 sponge and whose extension
is x^4 + 11; SP1's field under another width-16 permutation).  rk_rv32mem_journal_device under each set against numpy and
rk_rv32mem_journal_root; the nine device tables of every shard against numpy; the run end to end through the shard pool
(five shards, three in flight) and through the pipeline, whose witness context commits the digest; the pool's claims
routed to the shard they belong to; the unlinked set under risc0's preset.  Every comparison is bit-exact."""
import numpy as np
import pytest

import rv32_link_programs as LP
import rv32_mem_programs as GP
import test_rv32_link_runs as R
from test_gpu_rv32_link import INPUT
from raiko_amd import _lib, p3, rv32elf, rv32link, rv32mem, rv32_sets
from raiko_amd import executor as X
from raiko_amd import hal as H

pytestmark = pytest.mark.gpu

SETS = sorted(LP.LINK_SETS)
_cpu = {}


def _reference():
    """-> (elf, the CPU executor's run, program image, journals, final words by the plain-Python replay): made once"""
    if not _cpu:
        assert INPUT == R.T.INPUT
        elf, ex, image, _preps, journals, _mem_image = R.relay()
        memory = R.replayed_memory(elf, ex)
        _cpu["v"] = (elf, ex, image, journals, {int(w): memory[int(w)] for m in ex.mem for w in m[:, 1]})
    return _cpu["v"]


def _context(name):
    """a context under set `name` -> (HipHal, the blob applied)"""
    preset, over = LP.LINK_SETS[name]
    h = H.HipHal(0)
    try:
        return h, h.set_params(preset, **over)
    except Exception:
        h.close()
        raise


def _blob(name):
    preset, over = LP.LINK_SETS[name]
    return H.make_params(preset, **over)


# ------------------------------------------------------------------------------------------------ the digest kernel path
@pytest.mark.parametrize("name", SETS)
def test_journal_device_under_sets(name):
    _elf, ex, _image, journals, _final = _reference()
    tables = [rv32mem.memory_rows(m)[0] for m in ex.mem]
    big = X.execute(GP.count_program(300, distinct=True), INPUT, segment_limit_po2=13, record_trace=True)
    tables.append(rv32mem.memory_rows(big.mem[0])[0])
    assert tuple(t.shape[0] for t in tables) == LP.MEMORY_HEIGHTS + (512,)
    h, blob = _context(name)
    try:
        for k, t in enumerate(tables):
            lg = t.shape[0].bit_length() - 1
            want = rv32link.journal_of_table(t)
            assert k >= LP.N_SHARDS or np.array_equal(want, journals[k])
            buf = h.copy_from_elem(np.ascontiguousarray(p3.to_mont(t)).reshape(-1))
            h.sync()
            try:
                root, journal, link, n_real = rv32_sets.journal_device(h, buf, lg, keep=True)
            finally:
                buf.free()
            assert n_real == len(want) == int(t[:, rv32mem.B_REAL].sum())
            assert np.array_equal(journal, want)
            assert np.array_equal(link, rv32link.link_matrix(want, lg))
            assert np.array_equal(root, rv32link.journal_root(want, lg, blob)), (k, lg)
            if name != "sp1":                          # also for the empty journal: the all-zero subtrees hash differently
                assert not np.array_equal(root, rv32link.journal_root(want, lg, _blob("sp1"))), (k, lg)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ the witness
def test_relay_tables_equal_numpy():
    """all nine tables of all five shards as execute_rv32_device(link=True) writes them, their public values (the pcs,
    the registers, the digest at the 4-, 64- and 2-row heights) and the journals against numpy"""
    elf, ref_ex, image, want, _final = _reference()
    h, blob = _context("sp1")
    try:
        key = X.setup_rv32_elf(h, elf, blob, chips="rv32im-mem", link=True)
        try:
            ref = rv32_sets.shards("rv32im-mem", ref_ex, image, airs=key.airs, link=True, params=blob)
            ex, shards, _dev, bufs, journals = X.execute_rv32_device(h, elf, INPUT, LP.PO2, chips="rv32im-mem", key=key, link=True)
            try:
                h.sync()
                assert len(shards) == len(ref) == len(journals) == LP.N_SHARDS
                assert tuple(s.cycles for s in ex.segments) == LP.CYCLES
                for k, ((rt, rinit, rj), d, (tables, init), j) in enumerate(zip(ref, bufs, shards, journals)):
                    assert len(tables) == len(rt) == len(d) == 9 and np.array_equal(init, rinit)
                    assert np.array_equal(j, rj) and np.array_equal(j, want[k]) and j.shape == (LP.JOURNAL_ROWS[k], 3)
                    for i, (r, (b, lg), t) in enumerate(zip(rt, d, tables)):
                        assert lg == r.log_height == t.log_height, (k, i)
                        assert np.array_equal(b.to_host(), r.trace.reshape(-1)), (k, i)
                        assert np.array_equal(t.public_values, r.public_values), (k, i)
                    assert 1 << d[8][1] == LP.MEMORY_HEIGHTS[k]
                    assert np.array_equal(tables[8].public_values, rv32link.journal_root(want[k], d[8][1], blob))
            finally:
                for d in bufs:
                    for b, _lg in d:
                        b.free()
        finally:
            key.close()
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ end to end
_pool = {}


def _through_pool(name):
    """relay through execute_and_prove_p3 under set `name`, three proofs in flight -> (blob, ex, shards, proofs); the
    words are kept for the tests that compare runs, the contexts are the call's own and closed when it returns"""
    if name not in _pool:
        elf = _reference()[0]
        blob = _blob(name)
        ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=LP.PO2, params=blob, batch=3, chips="rv32im-mem", link=True)
        _pool[name] = (blob, ex, shards, proofs)
    return _pool[name]


def _vk(ex):
    return dict(prep_root=ex.prep_root, program_log_height=ex.program_log_height)


@pytest.mark.parametrize("name", SETS)
def test_relay_end_to_end(name):
    elf, _ref_ex, _image, want, final = _reference()
    blob, ex, shards, proofs = _through_pool(name)
    ex2, pproofs, _kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=LP.PO2, params=blob, chips="rv32im-mem", link=True)
    assert len(proofs) == len(pproofs) == LP.N_SHARDS and all(np.array_equal(a, b) for a, b in zip(proofs, pproofs))
    assert np.array_equal(ex.prep_root, ex2.prep_root)
    for e in (ex, ex2):
        assert len(e.journals) == LP.N_SHARDS and all(np.array_equal(a, b) for a, b in zip(e.journals, want))
        assert e.final_memory == final and len(final) == LP.TOUCHED_WORDS and final[(LP.DATA + 12) >> 2] == LP.FINAL_AT_12
    vk = _vk(ex)
    image = rv32link.memory_image(elf)
    entry = ex.segments[0].start_pc
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=entry, **vk, journals=ex.journals, image=image)
    for k, ((tables, init), pf) in enumerate(zip(shards, proofs)):
        assert 1 << int(pf[1 + rv32link.MEMORY_TABLE]) == LP.MEMORY_HEIGHTS[k]           # the height the digest is taken at
        assert np.array_equal(tables[8].public_values, rv32link.journal_root(want[k], tables[8].log_height, blob))
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=ex.journals[k]) == 0
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=ex.journals[(k + 1) % LP.N_SHARDS]) != 0
        # without claims: refused where the shard sent anything.  Shard 2 sent nothing: a linked proof with an empty
        # link bus balances on its own, and its empty journal adds a claim of no tuples
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk) == (0 if k == LP.EMPTY_SHARD else 8)
    # the chain check does not place the empty journal (tests/test_rv32_link_runs.py); the digests do
    swapped = [ex.journals[0], ex.journals[1], ex.journals[3], ex.journals[2], ex.journals[4]]
    assert rv32link.check_memory_chain(swapped, image) == final
    with pytest.raises(ValueError, match="shard 2: the proof does not verify"):
        X.verify_rv32_execution(shards, proofs, blob, entry_pc=entry, **vk, journals=swapped, image=image)


def test_a_proof_under_one_set_is_refused_under_the_other():
    """sp1 and m4_0_tables share field, extension, shapes and the guest: only the hash differs.  The statement of one
    run -- its tables, digests, root and blob -- with the proof of the other is refused, shard 0 each way"""
    runs = {name: _through_pool(name) for name in ("sp1", "m4_0_tables")}
    for mine, other in (("sp1", "m4_0_tables"), ("m4_0_tables", "sp1")):
        blob, ex, shards, proofs = runs[mine]
        _ob, oex, oshards, oproofs = runs[other]
        (tables, init), j = shards[0], ex.journals[0]
        assert np.array_equal(j, oex.journals[0]) and np.array_equal(init, oshards[0][1]) and proofs[0].size == oproofs[0].size
        assert not np.array_equal(ex.prep_root, oex.prep_root)
        assert not np.array_equal(tables[8].public_values, oshards[0][0][8].public_values)
        assert X.verify_rv32_shard(tables, proofs[0], init, blob, **_vk(ex), journal=j) == 0
        assert X.verify_rv32_shard(tables, oproofs[0], init, blob, **_vk(ex), journal=j) != 0
        # the other run's whole statement under this set's blob: the digest is not this hash's
        assert X.verify_rv32_shard(oshards[0][0], oproofs[0], init, blob, **_vk(oex), journal=j) == 2
        vt = X.rv32_verifier_tables(oshards[0][0], oproofs[0], **_vk(oex))
        assert p3.verify(vt, oproofs[0], init, blob, prep_root=oex.prep_root, claims=rv32link.claims_of(j)) != 0


def test_unlinked_mem_set_under_risc0():
    blob = H.make_params(0, **LP.FAST)
    elf = GP.two_shard_program()
    ex, shards, proofs = X.execute_and_prove_p3(elf, INPUT, shard_po2=13, params=blob, batch=2, chips="rv32im-mem")
    ex2, pproofs, _kept = X.execute_and_prove_p3_pipelined(elf, INPUT, shard_po2=13, params=blob, chips="rv32im-mem")
    assert len(proofs) == len(pproofs) == 2 and all(np.array_equal(a, b) for a, b in zip(proofs, pproofs))
    assert np.array_equal(ex.prep_root, ex2.prep_root)
    vk = _vk(ex)
    assert X.verify_rv32_execution(shards, proofs, blob, entry_pc=ex.segments[0].start_pc, **vk)
    sp1 = H.make_params(1, **LP.FAST)
    for (tables, init), pf in zip(shards, proofs):
        assert tables[8].public_values.size == 0
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk) == 0 != X.verify_rv32_shard(tables, pf, init, sp1, **vk)


# ------------------------------------------------------------------------------------------------ the pool's claims
def _numpy_run(h, blob, link):
    """-> (key, [(tables, init)], journals): relay's five numpy shards under a key on h"""
    elf, ex, image, _journals, _final = _reference()
    key = X.setup_rv32_elf(h, elf, blob, chips="rv32im-mem", link=link)
    try:
        made = rv32_sets.shards("rv32im-mem", ex, image, airs=key.airs, link=link, **(dict(params=blob) if link else {}))
    except Exception:
        key.close()
        raise
    return key, [m[:2] for m in made], [m[2] for m in made] if link else None


def _altered(claim):
    bus, sign, tuples = claim
    tuples = tuples.copy()
    tuples[0, 4] = p3.to_mont([(int(p3.from_mont(tuples[0, 4:5])[0]) + 1) % rv32mem.P])[0]
    return bus, sign, tuples


def test_pool_routes_claims_by_shard():
    """five shards, three proofs in flight: claims[i] reaches the verifier of shard i"""
    h, blob = _context("sp1")
    try:
        key, shards, journals = _numpy_run(h, blob, link=True)
        try:
            claims = [rv32link.claims_of(j) for j in journals]
            assert [c[0][2].shape for c in claims] == [(n, 6) for n in LP.JOURNAL_ROWS]
            run = lambda cl: p3.prove_shards(shards, blob, batch=3, verify=True, key=key.key, claims=cl)
            proofs = run(claims)
            vk = dict(prep_root=key.root, program_log_height=key.program_log_height)
            for (tables, init), pf, j in zip(shards, proofs, journals):
                assert X.verify_rv32_shard(tables, pf, init, blob, **vk, journal=j) == 0
            cases = {"altered": ([claims[0], claims[1], claims[2], [_altered(claims[3][0])], claims[4]], (3,)),
                     "ends exchanged": ([claims[4], claims[1], claims[2], claims[3], claims[0]], (0, 4)),
                     "the empty shard given the next one's": ([claims[0], claims[1], claims[3], claims[3], claims[4]], (2, 3))}
            assert claims[0][0][2].shape == claims[4][0][2].shape and not np.array_equal(claims[0][0][2], claims[4][0][2])
            for what, (cl, where) in cases.items():
                with pytest.raises(_lib.RkError) as e:
                    run(cl)
                assert e.value.status == _lib.RK_ERR_VERIFY and e.value.segment in where, what
        finally:
            key.close()
    finally:
        h.close()


def test_an_unlinked_proof_is_no_linked_proof():
    """shard 2 touches no memory: under the linked AIRs it sends nothing on the link bus, like the unlinked memory AIR.
    A proof of it made with the unlinked AIRs under the shared key is still no proof of the linked statement, whose
    memory table carries the digest as public values"""
    h, blob = _context("sp1")
    try:
        key, shards, _none = _numpy_run(h, blob, link=False)
        try:
            vk = dict(prep_root=key.root.copy(), program_log_height=key.program_log_height)
            tables, init = shards[LP.EMPTY_SHARD]
            pf = p3.prove(h, tables, init, key=key.key)
        finally:
            key.close()
        lkey, lshards, journals = _numpy_run(h, blob, link=True)
        try:
            assert np.array_equal(lkey.root, vk["prep_root"]) and lkey.program_log_height == vk["program_log_height"]
            ltables, linit = lshards[LP.EMPTY_SHARD]
            empty = journals[LP.EMPTY_SHARD]
            lpf = p3.prove(h, ltables, linit, key=lkey.key)
        finally:
            lkey.close()
        assert empty.shape == (0, 3) and np.array_equal(init, linit)
        assert all(np.array_equal(a.trace, b.trace) for a, b in zip(tables, ltables))
        assert X.verify_rv32_shard(tables, pf, init, blob, **vk) == 0
        assert X.verify_rv32_shard(ltables, lpf, linit, blob, **vk, journal=empty) == 0
        assert X.verify_rv32_shard(ltables, pf, linit, blob, **vk, journal=empty) != 0
        assert X.verify_rv32_shard(ltables, pf, linit, blob, **vk) != 0
        assert X.verify_rv32_shard(tables, lpf, init, blob, **vk) != 0
    finally:
        h.close()
