"""The FRI statements over proofs under a verifying key on the GPU (raiko_amd/fri_transcript.py with prep_root): keyed shard
proofs are made with p3.setup / p3.prove(key=...) from tests/p3_prep_cases.py, and the rows rk_fri_transcript_rows_device,
rk_fri_open_rows_device and rk_fri_reduce_rows_device write for them equal the numpy witness word for word; the statement's
proof over the on-device tables is the oracle's over the witness and is bound to the key's root; one rv32im-elf shard proof
goes through the same; bad arguments are refused with nothing written; and a statement captured through the _key entry
points with a NULL root writes the unkeyed statement's words.

Every GPU step runs in a child process of its own under a time limit of its own (this file run as a script: `python
tests/test_gpu_fri_key.py STEP [CASE [SET]]`, SET a parameter set of tests/fri_param_sets.py), once: a step that fails is not started again, and after a step that ended by a
signal or ran into its time limit no further step is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)          # run as a script: the package lies beside tests/
import fri_param_sets as PS  # noqa: E402
# gate_cubic     gate_table(6, 2, cubic=True) alone: the preprocessed tree at full height, a group of fewer than 8 cells
# gate_two       gate_table(5, 9) beside gate_table(8, 17): two preprocessed matrices of different heights -- an injection
#                inside the preprocessed tree --, groups of 9 and 17 cells (two and three sponge blocks)
# fib_gate_wide  a plain Fibonacci table of 2^9 rows beside gate_table(4, 42): log_kmax far below log_max, the program
#                table's width
# mix            mix_tables(6): lookups and preprocessed columns together, all four trees
ROW_CASES = ["gate_cubic", "gate_two", "fib_gate_wide", "mix"]
OVER = dict(queries=7, pow_bits=2)
_stop = []          # set by a step that faulted or hung: nothing more is started on the GPU


def run_step(step, case="", limit=300, pset=""):
    """pset: a parameter set of tests/fri_param_sets.py, "" = SP1's preset under OVER"""
    if _stop:
        pytest.fail("not started: the step %s ended abnormally before" % _stop[0])
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), step, case, pset], cwd=ROOT, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _stop.append(" ".join((step, case, pset)))
        pytest.fail("%s %s %s ran into its time limit of %d s" % (step, case, pset, limit))
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _stop.append(" ".join((step, case, pset)))
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("case", ROW_CASES)
def test_gpu_rows_equal_the_witness(case):
    assert "rows ok" in run_step("rows", case)


def test_gpu_keyed_rows_under_the_other_matrix():
    """the keyed transcript statement (a fourth input batch, the key's root absorbed first) with the <0> kernels and the K2 chain"""
    assert "rows ok" in run_step("rows", PS.KEYED_CASE, pset=PS.KEYED_SET)


def test_gpu_proves_the_statement_bound_to_the_key():
    assert "proof ok" in run_step("prove", "mix", limit=600)


def test_gpu_elf_shard_proof_through_the_transcript_statement():
    """one rv32im-elf shard proof (tests/rv32_chip_programs.py alu_program, the first shard) at queries=7: the byte table
    makes log_max 19; the numpy witness of the statement takes a few seconds at that shape (it walks queries x columns
    and queries x tree levels, not the tables' rows), so every table is compared whole"""
    assert "elf ok" in run_step("elf", "", limit=600)


def test_gpu_bad_arguments_are_refused_with_nothing_written():
    assert "refusals ok" in run_step("refuse", "mix")


def test_gpu_null_root_statement_writes_the_unkeyed_words():
    assert "unchanged ok" in run_step("unchanged", "sp1_lookup_beside_plain")


# ---------------------------------------------------------------------------------------------- the steps (child process)
def _tables(case):
    import p3_prep_cases as K
    from raiko_amd import p3
    if case == "gate_cubic":
        return [K.gate_table(6, 2, cubic=True)]
    if case == "gate_two":
        return [K.gate_table(5, 9), K.gate_table(8, 17)]
    if case == "fib_gate_wide":
        return [p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(9)), K.gate_table(4, 42)]
    return K.mix_tables(6)


def _keyed_shard(h, case, **more):
    """-> (blob, full tables, verifier's tables, init, proof, root): a shard proof under a key made here"""
    import oracle_lib as o
    import p3_prep_cases as K
    from raiko_amd import p3
    over = dict(OVER, **more)
    blob = h.set_params(1, **over)
    o.oracle_set_params(1, **over)
    assert h.get_params().p2_m4 == blob.p2_m4
    tables, init = _tables(case), p3.to_mont([167009, 10, 3])
    key = p3.setup(h, tables)
    try:
        pf = p3.prove(h, tables, init, key=key)
        root = key.root.copy()
    finally:
        key.close()
    ver = K.pinned(tables)
    assert p3.verify(ver, pf, init, params=blob, prep_root=root) == 0
    return blob, tables, ver, init, pf, root


def _same(dev, want):
    import numpy as np
    assert len(dev) == len(want)
    for k, ((buf, lh), w) in enumerate(zip(dev, want)):
        assert (1 << lh) == w.shape[0], (k, lh, w.shape)
        got = buf.to_host().reshape(w.shape)
        assert np.array_equal(got, w), (k, np.argwhere(got != w)[:8])


def step_rows(h, case, pset=""):
    from raiko_amd import fri_open as H, fri_reduce as G, fri_transcript as X, p3
    blob, tables, ver, init, pf, root = _keyed_shard(h, case, **(PS.PARAM_SETS[pset][1] if pset else {}))
    assert not pset or blob.p2_m4 == PS.PARAM_SETS[pset][1]["p2_m4"]
    st = X.statement(ver, pf, init, blob, prep_root=root)
    opn, sh = st.opn, st.shape
    hts = {t.batch: t.B for t in opn.trees}
    cells = sorted(g.cells for g in opn.groups if g.batch == 3)
    kt = next(t for t in opn.trees if t.batch == 3)
    assert 3 <= min(m.log_n for m in opn.layout) and sh.log_max <= 10
    if case == "gate_cubic":
        assert hts == {0: sh.log_max, 2: sh.log_max, 3: sh.log_max} and cells == [2]
    elif case == "gate_two":
        assert hts[3] == sh.log_max and cells == [9, 17] and sum(v is not None for v in kt.group_at) == 1
    elif case == "fib_gate_wide":
        assert hts[3] == 5 and sh.log_max == 10 and cells == [42] and 1 not in hts
    else:
        assert sorted(hts) == [0, 1, 2, 3]
    sz = X.sizes(st)
    assert sz["roots_words"] == 34 and sz["log_kmax"] == opn.log_kmax == hts[3] and sz["n_batches"] == len(hts)
    want = [p3.to_mont(r) for r in X.witness(st)]
    _same(X.device_tables(h, st), want)
    assert [w.shape[0] for w in want] == [1 << v for v in X.heights(st)]
    _same(H.device_tables(h, opn), [p3.to_mont(r) for r in H.witness(opn)])
    _same(G.device_tables(h, st.red), [p3.to_mont(r) for r in G.witness(st.red)])
    print("rows ok")


def step_prove(h, case):
    import numpy as np
    import oracle_lib as o
    import p3_prep_cases as K
    from raiko_amd import fri_transcript as X, p3
    blob, tables, ver, init, pf, root = _keyed_shard(h, case, queries=100)
    st = X.statement(ver, pf, init, blob, prep_root=root)
    assert st.shape.queries == 100 and len(st.opn.trees) == 4
    dev = X.device_tables(h, st)
    host = X.host_tables(st)
    for (buf, lh), t in zip(dev, host):
        assert np.array_equal(buf.to_host().reshape(t.trace.shape), t.trace)
    got = X.prove(h, st, dev)
    assert np.array_equal(got, o.oracle_p3_prove(host, st.init))
    assert p3.verify(host, got, st.init, params=blob) == 0
    assert X.verify_transcript_statement(ver, pf, init, got, blob, prep_root=root) == 0
    forged = [K.with_prep_cell_changed(tables[0], row=3, col=1)] + tables[1:]
    other = p3.setup(h, forged)
    try:
        assert not np.array_equal(other.root, root)
        assert X.verify_transcript_statement(ver, pf, init, got, blob, prep_root=other.root.copy()) != 0
    finally:
        other.close()
    print("proof ok")


def step_elf(h, case):
    import numpy as np
    import rv32_chip_programs as CP
    from raiko_amd import executor as E, fri_transcript as X, hal, p3
    par = hal.make_params(1, **OVER)
    ex, shards, proofs = E.execute_and_prove_p3(CP.alu_program(1), [11, 22, 33, 44], shard_po2=13, params=par, chips="rv32im-elf")
    tables, init = shards[0]
    pf = proofs[0]
    ver = E.rv32_verifier_tables(tables, pf, ex.prep_root, ex.program_log_height)
    assert ver is not None and p3.verify(ver, pf, init, par, prep_root=ex.prep_root) == 0
    blob = h.set_params(1, **OVER)
    st = X.statement(ver, pf, init, blob, prep_root=ex.prep_root)
    assert st.shape.log_max == 19 and st.shape.queries == 7 and sum(m.batch == 3 for m in st.opn.layout) == 4
    sz = X.sizes(st)
    assert sz["log_kmax"] == 19 and sz["n_batches"] == 4
    dev = X.device_tables(h, st)
    _same(dev, [p3.to_mont(r) for r in X.witness(st)])
    got = X.prove(h, st, dev)
    assert p3.verify(X._pinned_tables(st), got, st.init, params=blob) == 0
    assert X.verify_transcript_statement(ver, pf, init, got, blob, prep_root=ex.prep_root) == 0
    bad = ex.prep_root.copy()
    bad[5] = (int(bad[5]) + 1) % p3.P
    assert X.verify_transcript_statement(ver, pf, init, got, blob, prep_root=bad) != 0
    print("elf ok")


def step_refuse(h, case):
    import numpy as np
    from raiko_amd import _lib, fri_transcript as X, p3
    from raiko_amd.hal import _ptr
    blob, tables, ver, init, pf, root = _keyed_shard(h, case)
    st = X.statement(ver, pf, init, blob, prep_root=root)
    sz = X.sizes(st)
    assert sz["n_batches"] == 4 and sz["roots_words"] == 34
    words = [sz[n + "_width"] << sz[n + "_log_height"] for n in X.TABLE_NAMES]
    mark = [np.full(w, 0x5A5A5A5A, dtype=np.uint32) for w in words]
    bufs = [h.copy_from_elem(m) for m in mark]
    in_bufs = [h.copy_from_elem(a) for a in X.device_inputs(st)]     # kept: the calls below read them
    ins = [_ptr(b) for b in in_bufs]
    assert len(ins) == 7 and len(bufs) == 8
    lib = _lib.load()
    sh = st.shape
    lw, ow = st.opn.layout_words, st.ops_words
    lp, nm, op, no = lw.ctypes.data_as(_lib.u32p), len(st.opn.layout), ow.ctypes.data_as(_lib.u32p), len(st.ops)
    full = []
    for k, b in enumerate(bufs):
        full += [_ptr(b), words[k]]
    fn = lib.rk_fri_transcript_rows_device
    for short in range(8):
        args = list(full)
        args[2 * short + 1] -= 1
        assert fn(h._ctx, sh.log_max, sh.blowup_log2, sh.queries, lp, nm, op, no, *ins, *args) == _lib.RK_ERR_CAPACITY
    call = lambda bl, layout, n, inputs: fn(h._ctx, sh.log_max, bl, sh.queries, layout, n, op, no, *inputs, *full)
    for k in range(7):
        assert call(sh.blowup_log2, lp, nm, [None if j == k else v for j, v in enumerate(ins)]) == _lib.RK_ERR_INVALID
    assert call(sh.blowup_log2, None, nm, ins) == _lib.RK_ERR_INVALID
    bad = np.array(st.opn.layout, dtype=np.uint64).reshape(-1, 5)
    k3 = int(np.argmax(bad[:, 0] == 3))
    bad[k3, 3] = 1                                                                      # one point on a preprocessed matrix
    assert call(sh.blowup_log2, p3.to_mont(bad.reshape(-1)).ctypes.data_as(_lib.u32p), nm, ins) == _lib.RK_ERR_INVALID
    h.set_params(1, **dict(OVER, blowup_log2=2))                                        # the keyed layout, the context under another blow-up
    assert call(sh.blowup_log2, lp, nm, ins) == _lib.RK_ERR_INVALID
    h.sync()
    for b, m in zip(bufs, mark):
        assert np.array_equal(b.to_host(), m)
    h.set_params(1, **OVER)
    assert call(sh.blowup_log2, lp, nm, ins) == 0
    h.sync()
    for b, w in zip(bufs, X.witness(st)):
        assert np.array_equal(b.to_host().reshape(w.shape), p3.to_mont(w))
    del in_bufs
    print("refusals ok")


def step_unchanged(h, case):
    import numpy as np
    import oracle_lib as o
    from p3_cases import P3_CASES, init_of, tables_of
    from raiko_amd import fri_chip as F, fri_open as H, fri_reduce as G, fri_tables as T, fri_transcript as X, p3
    preset, over, _, _ = P3_CASES[case]
    blob = h.set_params(preset, **over)
    o.oracle_set_params(preset, **over)
    tables, init = tables_of(case), init_of(case)
    pf = p3.prove(h, tables, init)
    plain = X.statement(tables, pf, init, blob)
    cap = lambda name, n: T.capture(name + "_key", n, tables, pf, init, blob)           # the _key twin, a NULL root
    (rc, shape, pub, rec), (rc2, _, layout, in_pub, in_rec) = cap("rk_p3_fri_openings", 2), cap("rk_p3_fri_inputs", 3)
    (rc3, _, roots, paths), (rc4, _, ops, obs, smp) = cap("rk_p3_fri_input_paths", 2), cap("rk_p3_fri_transcript", 3)
    assert (rc, rc2, rc3, rc4) == (0, 0, 0, 0) and roots.size == 25
    lay = [G.Matrix(*[int(v) for v in row]) for row in p3.from_mont(layout).reshape(-1, 5)]
    keyed = X.Statement(H.Statement(G.Statement(F.Statement(shape, pub, rec, blob), lay, in_pub, in_rec, blob), roots, paths), ops, obs, smp)
    a = [b.to_host() for b, _ in X.device_tables(h, plain)]
    b = [b.to_host() for b, _ in X.device_tables(h, keyed)]
    assert len(a) == len(b) == 8
    for x, y in zip(a, b):
        assert x.any() and np.array_equal(x, y)
    assert X.sizes(plain) == X.sizes(keyed) and X.sizes(keyed)["log_kmax"] == 0
    print("unchanged ok")


def main(step, case="", pset=""):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as o
    from raiko_amd import hal
    h = hal.HipHal(0)
    try:
        {"rows": step_rows, "prove": step_prove, "elf": step_elf, "refuse": step_refuse, "unchanged": step_unchanged}[step](h, case, *([pset] if pset else []))
    finally:
        o.oracle_set_params()
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
