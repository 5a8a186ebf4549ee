"""rk_fri_transcript_rows_device on the GPU (raiko_amd/fri_transcript.py): the rows of fold'', path, reduce'', ipath, transcript,
bits, chip and the state chip equal the numpy witness word for word -- the challenger's chain walked by one wave, one lane per
state cell --; the tables stay in HBM and go to rk_p3_prove as on_device tables, whose proof is the oracle's over the
witness; verify_transcript_statement accepts it; undersized, null, ill-planned or wrong-parameter calls are refused with
nothing written; the six tables shared with the open statement hold the same words whichever call wrote them.

Every GPU step runs in a child process of its own under a time limit of its own (this file run as a script: `python
tests/test_gpu_fri_transcript.py STEP [CASE [SET]]`, SET a parameter set of tests/fri_param_sets.py), once: a step that fails is not started again, and after a step that ended
by a signal or ran into its time limit no further step is started."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)          # run as a script: the package lies beside tests/
import fri_param_sets as PS  # noqa: E402
# the cases of tests/test_fri_transcript.py: (queries, init, further overrides) per case of tests/test_gpu_fri_open.py --
# 7, 8 and 100 queries (the indices end with the proof-of-work block; one duplex that absorbs nothing; twelve), with and
# without a permutation batch, an empty init, pow_bits = 0
ROW_CASES = {"sp1_mixed_fib8_cubic4": (7, [5, 6, 7], {}), "sp1_same_height": (100, [], dict(pow_bits=0)), "sp1_lookup_beside_plain": (8, [1, 2, 3, 4, 5], {}),
             "sp1_blow2_wide_k9": (7, [11, 12], {}), "sp1_width_301": (8, [], {}), "sp1_tiny_beside_tall": (8, [2, 3], {}),
             "sp1_twelve_tables": (7, [1], {})}
_stop = []          # set by a step that faulted or hung: nothing more is started on the GPU


def run_step(step, case="", limit=300, pset=""):
    """pset: a parameter set of tests/fri_param_sets.py, "" = the case's own parameters"""
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


@pytest.mark.parametrize("case", list(ROW_CASES))
def test_gpu_rows_equal_the_witness(case):
    assert "rows ok" in run_step("rows", case)


@pytest.mark.parametrize("pset,case", PS.ROW_IDS, ids=[PS.row_id(*x) for x in PS.ROW_IDS])
def test_gpu_rows_under_parameter_sets(pset, case):
    """every two-instantiation kernel of csrc/fri_tables.hip under both external matrices -- fri_path_kernel, fri_open_sponge_kernel,
    fri_open_ipath_kernel <0> and <1>, fri_transcript_chain_kernel<K2> and <K3> --, other tables, another field, blow-ups 8 and 16"""
    assert "rows ok" in run_step("rows", case, pset=pset)


@pytest.mark.parametrize("pset", PS.PROVE_SETS)
def test_gpu_proves_the_statement_under_parameter_sets(pset):
    """the statement proven from device tables at the case's own small query count, interpreted and compiled"""
    assert "proof ok" in run_step("prove", PS.PROVE_CASE, pset=pset)


def test_gpu_proves_the_statement_from_device_tables():
    """SP1's 100 queries over a 2^11-row shard (the shape of tests/test_gpu_fri_open.py)"""
    assert "proof ok" in run_step("prove", "sp1_tiny_beside_tall", limit=600)


def test_gpu_bad_arguments_are_refused_with_nothing_written():
    assert "refusals ok" in run_step("refuse", "sp1_mixed_fib8_cubic4")


def test_gpu_shared_tables_are_the_same_words_in_both_statements():
    assert "shared ok" in run_step("shared", "sp1_mixed_fib8_cubic4")


def test_gpu_shared_tables_are_the_same_words_under_the_other_matrix():
    assert "shared ok" in run_step("shared", PS.SHARED_CASE, pset=PS.SHARED_SET)


# ---------------------------------------------------------------------------------------------- the steps (child process)
def _shard(h, case, queries=None, init=None, pset="", **more):
    import numpy as np
    import oracle_lib as o
    from p3_cases import P3_CASES, tables_of
    from raiko_amd import p3
    if pset:
        assert queries is None and init is None
        preset, over = PS.shard_params(pset, case, transcript=True)
        tables, iw = PS.shard_tables(pset, case, transcript=True)
        over = dict(over, **more)
    else:
        q, i, m = ROW_CASES[case]
        preset, over, _, _ = P3_CASES[case]
        over = dict(over, queries=q if queries is None else queries, **dict(m, **more))
        tables, iw = tables_of(case), p3.to_mont(np.array(i if init is None else init, dtype=np.uint64))
    blob = h.set_params(preset, **over)
    o.oracle_set_params(preset, **over)
    got = h.get_params()
    assert (got.p2_m4, got.ext_w, got.blowup_log2) == (blob.p2_m4, blob.ext_w, blob.blowup_log2)
    return blob, tables, iw, p3.prove(h, tables, iw), (preset, over)


def step_rows(h, case, pset=""):
    import numpy as np
    import oracle_lib as o
    from raiko_amd import fri_transcript as X, p3
    blob, tables, init, pf, _ = _shard(h, case, pset=pset)
    assert np.array_equal(pf, o.oracle_p3_prove(tables, init))
    st = X.statement(tables, pf, init, blob)
    want = [p3.to_mont(r) for r in X.witness(st)]
    dev = X.device_tables(h, st)
    assert [lh for _, lh in dev] == list(X.heights(st))
    for (buf, lh), w in zip(dev, want):
        got = buf.to_host().reshape(w.shape)
        assert np.array_equal(got, w), np.argwhere(got != w)[:8]
    print("rows ok")


def step_prove(h, case, pset=""):
    """pset: under a parameter set, at the shard's own query count and with compiled AIRs too; else SP1's 100 queries"""
    import numpy as np
    import oracle_lib as o
    from raiko_amd import fri_transcript as X, p3
    blob, tables, init, pf, _ = _shard(h, case, pset=pset) if pset else _shard(h, case, queries=100)
    st = X.statement(tables, pf, init, blob)
    sz = X.sizes(st)
    assert pset or sz["path_rows"] >= 1 << 12 and sz["bits_rows"] == 101 and sz["state_rows"] == 100 * 4 + sz["n_steps"] and sz["n_steps"] < 100
    dev = X.device_tables(h, st)
    host = X.host_tables(st)
    for (buf, lh), t in zip(dev, host):
        assert np.array_equal(buf.to_host().reshape(t.trace.shape), t.trace)
    got = X.prove(h, st, dev)
    assert np.array_equal(got, o.oracle_p3_prove(host, st.init))
    assert p3.verify(host, got, st.init, params=blob) == 0
    assert X.verify_transcript_statement(tables, pf, init, got, blob) == 0
    if pset:
        for air in X.airs(st):
            air.compile(h)
        again = X.prove(h, st, dev)
        assert np.array_equal(again, got) and p3.verify(host, again, st.init, params=blob) == 0
        assert X.verify_transcript_statement(tables, pf, init, again, blob) == 0
    assert np.array_equal(X.prove(h, st), got)                 # rows written anew
    print("proof ok")


def step_refuse(h, case):
    import numpy as np
    from raiko_amd import _lib, fri_transcript as X, p3
    from raiko_amd.hal import _ptr
    blob, tables, init, pf, (preset, over) = _shard(h, case)
    st = X.statement(tables, pf, init, blob)
    sz = X.sizes(st)
    words = [sz[n + "_width"] << sz[n + "_log_height"] for n in X.TABLE_NAMES]
    mark = [np.full(w, 0x5A5A5A5A, dtype=np.uint32) for w in words]
    bufs = [h.copy_from_elem(m) for m in mark]
    in_bufs = [h.copy_from_elem(a) for a in X.device_inputs(st)]     # kept: the calls below read them
    ins = [_ptr(b) for b in in_bufs]
    lib = _lib.load()
    sh = st.shape
    lw, ow = st.opn.layout_words, st.ops_words
    u = lambda a: a.ctypes.data_as(_lib.u32p)
    lp, nm, op, no = u(lw), len(st.opn.layout), u(ow), len(st.ops)
    full = []
    for k, b in enumerate(bufs):
        full += [_ptr(b), words[k]]
    for short in range(8):
        args = list(full)
        args[2 * short + 1] -= 1
        assert lib.rk_fri_transcript_rows_device(h._ctx, sh.log_max, sh.blowup_log2, sh.queries, lp, nm, op, no, *ins, *args) == _lib.RK_ERR_CAPACITY
    call = lambda lm, bl, q, layout, n, ops, n_ops, inputs: lib.rk_fri_transcript_rows_device(h._ctx, lm, bl, q, layout, n, ops, n_ops, *inputs, *full)
    L, B, Q = sh.log_max, sh.blowup_log2, sh.queries
    assert call(L, B + 1, Q, lp, nm, op, no, ins) == -1               # not the layout's blow-up
    assert call(L + 1, B, Q, lp, nm, op, no, ins) == -1               # a layout of another shape
    assert call(L, B, Q, None, nm, op, no, ins) == -1
    assert call(L, B, Q, lp, nm, None, no, ins) == -1
    assert call(L, B, Q + 1, lp, nm, op, no, ins) == -1               # calls that do not fit the shape: one sample_bits short
    assert call(L, B, Q, lp, nm, op, no - 1, ins) == -1
    late = ow.copy()
    late[-2:], late[-4:-2] = p3.to_mont([X.OBSERVE, 1]), ow[-2:]      # an observe behind a sample_bits
    assert call(L, B, Q, lp, nm, u(late), no, ins) == -1
    other = ow.copy()
    other[-1] = p3.to_mont([L - 1])[0]                                # an index of another length
    assert call(L, B, Q, lp, nm, u(other), no, ins) == -1
    for k in range(7):
        assert call(L, B, Q, lp, nm, op, no, [None if j == k else v for j, v in enumerate(ins)]) == -1
    h.set_params(1, queries=Q, pow_bits=7, blowup_log2=2)             # a blow-up that is not the context's
    assert call(L, B, Q, lp, nm, op, no, ins) == -1
    h.set_params(0)                                                   # the width-24 instance: outside the scope
    assert call(L, 2, Q, lp, nm, op, no, ins) == -1
    h.set_params(preset, **dict(over, p2_pad_free=0))                 # a sponge that pads: outside the scope
    assert call(L, B, Q, lp, nm, op, no, ins) == -1
    h.sync()
    for b, m in zip(bufs, mark):
        assert np.array_equal(b.to_host(), m)
    h.set_params(preset, **over)
    assert call(L, B, Q, lp, nm, op, no, ins) == 0
    h.sync()
    for b, w in zip(bufs, X.witness(st)):
        assert np.array_equal(b.to_host().reshape(w.shape), p3.to_mont(w))
    del in_bufs
    print("refusals ok")


def step_shared(h, case, pset=""):
    """the rows of the open and the transcript statement written one after the other on one context: what they share is
    written by one stage of the library (csrc/fri_tables.hip), so it is the same words in both -- compared table against
    table, without the numpy witness"""
    import numpy as np
    from raiko_amd import fri_open as H, fri_transcript as X
    blob, tables, init, pf, _ = _shard(h, case, pset=pset)
    st = X.statement(tables, pf, init, blob)
    rows = lambda names, dev: {n: b.to_host().reshape(1 << lh, -1) for n, (b, lh) in zip(names, dev)}
    opn = rows(H.TABLE_NAMES, H.device_tables(h, st.opn))
    trn = rows(X.TABLE_NAMES, X.device_tables(h, st))
    assert opn["fold"].any() and opn["reduce"].any() and opn["ipath"].any() and trn["transcript"].any() and trn["bits"].any()
    for n in ("path", "reduce", "ipath", "chip"):
        assert np.array_equal(trn[n], opn[n]), n
    assert np.array_equal(trn["fold"][:, :-1], opn["fold"])                 # fold'' = fold' | FIRST
    first = np.zeros(trn["fold"].shape[0], dtype=bool)
    first[: st.shape.queries * st.shape.n_rounds: st.shape.n_rounds] = True
    assert np.array_equal(trn["fold"][:, -1] != 0, first)
    n_sponge = H.sizes(st.opn)["state_rows"]
    assert np.array_equal(trn["state"][:n_sponge], opn["state"][:n_sponge])   # the sponge's permutations, then the transcript's
    assert trn["state"][n_sponge: n_sponge + len(st.plan.steps), -1].all() and not trn["state"][n_sponge + len(st.plan.steps):, -1].any()
    print("shared ok")


def main(step, case="", pset=""):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as o
    from raiko_amd import hal
    h = hal.HipHal(0)
    try:
        {"rows": step_rows, "prove": step_prove, "refuse": step_refuse, "shared": step_shared}[step](h, case, *([pset] if pset else []))
    finally:
        o.oracle_set_params()
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
