"""rk_fri_reduce_rows_device on the GPU (raiko_amd/fri_reduce.py): the rows of fold', path, reduce and chip equal the numpy
witness word for word; the tables stay in HBM and go to rk_p3_prove as on_device tables, whose proof is the oracle's over
the witness; verify_reduce_statement accepts it; undersized or wrong-parameter calls are refused with nothing written.

Every GPU step runs in a child process of its own under a time limit of its own (this file run as a script: `python
tests/test_gpu_fri_reduce.py STEP [CASE [SET]]`, SET a parameter set of tests/fri_param_sets.py), once: a step that fails is not started again, and after a step that ended by a
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
ROW_CASES = ["sp1_mixed_fib8_cubic4", "sp1_same_height", "sp1_lookup_beside_plain", "sp1_blow2_wide_k9"]
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


# 301 columns: more than the reduce kernel's workgroup takes at once (carry across waves and across pieces)
@pytest.mark.parametrize("case", ROW_CASES + ["sp1_width_301"])
def test_gpu_rows_equal_the_witness(case):
    assert "rows ok" in run_step("rows", case)


@pytest.mark.parametrize("pset,case", PS.ROW_IDS, ids=[PS.row_id(*x) for x in PS.ROW_IDS])
def test_gpu_rows_under_parameter_sets(pset, case):
    """fri_path_kernel<0> and <1>, the chip under other tables, shiftm, wm and gen_l of another field in the fold and reduce lanes, blow-ups 8 and 16"""
    assert "rows ok" in run_step("rows", case, pset=pset)


@pytest.mark.parametrize("pset", PS.PROVE_SETS)
def test_gpu_proves_the_statement_under_parameter_sets(pset):
    """the statement proven from device tables at the case's own small query count, interpreted and compiled"""
    assert "proof ok" in run_step("prove", PS.PROVE_CASE, pset=pset)


def test_gpu_proves_the_statement_from_device_tables():
    """SP1's 100 queries over a 2^11-row shard (the shape of tests/test_gpu_fri_chip.py)"""
    assert "proof ok" in run_step("prove", "sp1_tiny_beside_tall", limit=600)


def test_gpu_bad_arguments_are_refused_with_nothing_written():
    assert "refusals ok" in run_step("refuse", "sp1_mixed_fib8_cubic4")


# ---------------------------------------------------------------------------------------------- the steps (child process)
def _shard(h, case, pset="", **more):
    import fri_param_sets as PS
    import oracle_lib as o
    from p3_cases import P3_CASES, init_of, tables_of
    from raiko_amd import p3
    if pset:
        preset, over = PS.shard_params(pset, case)
        tables, init = PS.shard_tables(pset, case)
    else:
        preset, over, _, _ = P3_CASES[case]
        tables, init = tables_of(case), init_of(case)
    over = dict(over, **more)
    blob = h.set_params(preset, **over)
    o.oracle_set_params(preset, **over)
    got = h.get_params()
    assert (got.p2_m4, got.ext_w, got.blowup_log2) == (blob.p2_m4, blob.ext_w, blob.blowup_log2)
    return blob, tables, init, p3.prove(h, tables, init)


def step_rows(h, case, pset=""):
    import numpy as np
    import oracle_lib as o
    from raiko_amd import fri_reduce as G, p3
    blob, tables, init, pf = _shard(h, case, pset=pset)
    assert np.array_equal(pf, o.oracle_p3_prove(tables, init))
    st = G.statement(tables, pf, init, blob)
    want = [p3.to_mont(r) for r in G.witness(st)]
    dev = G.device_tables(h, st)
    assert [lh for _, lh in dev] == list(G.heights(st))
    for (buf, lh), w in zip(dev, want):
        got = buf.to_host().reshape(w.shape)
        assert np.array_equal(got, w), np.argwhere(got != w)[:8]
    print("rows ok")


def step_prove(h, case, pset=""):
    """pset: under a parameter set, at the case's own query count; else SP1's 100 queries"""
    import numpy as np
    import oracle_lib as o
    from raiko_amd import fri_reduce as G, p3
    blob, tables, init, pf = _shard(h, case, pset=pset) if pset else _shard(h, case, queries=100)
    st = G.statement(tables, pf, init, blob)
    sz = G.sizes(st)
    assert pset or sz["path_rows"] >= 1 << 12 and sz["reduce_rows"] == 100 * sz["rows_per_query"]
    dev = G.device_tables(h, st)
    host = G.host_tables(st)
    for (buf, lh), t in zip(dev, host):
        assert np.array_equal(buf.to_host().reshape(t.trace.shape), t.trace)
    got = G.prove(h, st, dev)
    assert np.array_equal(got, o.oracle_p3_prove(host, st.init))
    assert p3.verify(host, got, st.init, params=blob) == 0
    assert G.verify_reduce_statement(tables, pf, init, got, blob) == 0
    for air in G.airs(st):
        air.compile(h)
    again = G.prove(h, st, dev)
    assert np.array_equal(again, got) and p3.verify(host, again, st.init, params=blob) == 0
    assert G.verify_reduce_statement(tables, pf, init, again, blob) == 0
    assert np.array_equal(G.prove(h, st), got)                 # rows written anew
    print("proof ok")


def step_refuse(h, case):
    import numpy as np
    from raiko_amd import _lib, fri_reduce as G, p3
    from raiko_amd.hal import _ptr
    blob, tables, init, pf = _shard(h, case)
    st = G.statement(tables, pf, init, blob)
    sz = G.sizes(st)
    words = [sz[n + "_width"] << sz[n + "_log_height"] for n in G.TABLE_NAMES]
    mark = [np.full(w, 0x5A5A5A5A, dtype=np.uint32) for w in words]
    bufs = [h.copy_from_elem(m) for m in mark]
    in_bufs = [h.copy_from_elem(a) for a in (st.fold.publics, st.fold.records, st.reduce_publics, st.in_records)]   # kept: the calls below read them
    ins = [_ptr(b) for b in in_bufs]
    lib = _lib.load()
    sh = st.shape
    lw = st.layout_words
    lp, nm = lw.ctypes.data_as(_lib.u32p), len(st.layout)
    full = []
    for k, b in enumerate(bufs):
        full += [_ptr(b), words[k]]
    for short in range(4):
        args = list(full)
        args[2 * short + 1] -= 1
        assert lib.rk_fri_reduce_rows_device(h._ctx, sh.log_max, sh.blowup_log2, sh.queries, lp, nm, *ins, *args) == _lib.RK_ERR_CAPACITY
    call = lambda lm, bl, q, layout, n, inputs: lib.rk_fri_reduce_rows_device(h._ctx, lm, bl, q, layout, n, *inputs, *full)
    assert call(sh.log_max, sh.blowup_log2 + 1, sh.queries, lp, nm, ins) == -1          # not the layout's blow-up
    assert call(sh.log_max + 1, sh.blowup_log2, sh.queries, lp, nm, ins) == -1          # a layout of another shape
    assert call(sh.log_max, sh.blowup_log2, sh.queries, None, nm, ins) == -1
    bad = np.array(st.layout, dtype=np.uint64).reshape(-1)
    bad[2] = 0                                                                          # a matrix without columns
    assert call(sh.log_max, sh.blowup_log2, sh.queries, p3.to_mont(bad).ctypes.data_as(_lib.u32p), nm, ins) == -1
    for k in range(4):
        assert call(sh.log_max, sh.blowup_log2, sh.queries, lp, nm, [None if j == k else v for j, v in enumerate(ins)]) == -1
    h.set_params(1, queries=sh.queries, pow_bits=7, blowup_log2=2)                     # a blow-up that is not the context's
    assert call(sh.log_max, sh.blowup_log2, sh.queries, lp, nm, ins) == -1
    h.set_params(0)                                                                     # the width-24 instance: outside the scope
    assert call(sh.log_max, 2, sh.queries, lp, nm, ins) == -1
    h.sync()
    for b, m in zip(bufs, mark):
        assert np.array_equal(b.to_host(), m)
    from p3_cases import P3_CASES
    h.set_params(P3_CASES[case][0], **P3_CASES[case][1])
    assert call(sh.log_max, sh.blowup_log2, sh.queries, lp, nm, ins) == 0
    h.sync()
    for b, w in zip(bufs, G.witness(st)):
        assert np.array_equal(b.to_host().reshape(w.shape), p3.to_mont(w))
    del in_bufs
    print("refusals ok")


def main(step, case="", pset=""):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as o
    from raiko_amd import hal
    h = hal.HipHal(0)
    try:
        {"rows": step_rows, "prove": step_prove, "refuse": step_refuse}[step](h, case, *([pset] if pset else []))
    finally:
        o.oracle_set_params()
        h.close()
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
