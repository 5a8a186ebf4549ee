"""rk_p3_prove_shards_key: the shard pool under a key, at the smallest shapes with preprocessed columns
(p3_prep_cases.mix_tables(6), p3.lookup_demo_tables_prep(6), a gate_table(3, 5, True)).  Five shards with different traces
under one key, 1, 2 and 3 proofs in flight, host and device traces: every proof is word-identical to
p3.prove(hal, tables, init, key=key) on a single context -- the path tests/test_gpu_p3_prep.py holds to the exact
reference tests/p3_ref_prep.py -- and one pool proof per shape goes through that reference directly.  A shard that breaks
a constraint through a preprocessed column is RK_ERR_VERIFY with its index; keys and shards that do not fit are
RK_ERR_INVALID with no proof buffer touched; a key over tables without preprocessed columns gives rk_p3_prove_shards'
words.  Not exercised: multi-GPU runs of the keyed pool, and the two refusals that need a second GPU to reach (a key of
another device than its slot's, keys whose roots differ from each other).  One GPU here."""
import ctypes as C

import numpy as np
import pytest

import p3_prep_cases as K
import p3_ref as R
import p3_ref_prep as RP
from raiko_amd import _lib, hal as H, p3

pytestmark = pytest.mark.gpu
FAST = dict(queries=8, pow_bits=6)
BLOW = 1
N_SHARDS = 5


def _init(s):
    return p3.to_mont([20241, 7 + s])


def _gate_shard(s, air=K.gate_air(5, True)):
    """gate_table(3, 5, True)'s preprocessed matrix under a main trace that starts from x = s + 1"""
    base = K.gate_table(3, 5, True, seed=4, air=air)
    sm = p3.from_mont(base.prep).astype(object)
    n = sm.shape[0]
    t = np.zeros((n, 3), dtype=object)
    x = s + 1
    for r in range(n):
        y = (int(sm[r][0]) * x + sum(int(v) for v in sm[r][1:])) % K.P
        t[r] = [x, y, int(sm[r][0]) * x * y % K.P]
        x = (x + int(sm[(r + 1) % n][4])) % K.P
    assert air.check_trace(t, (), prep=sm) == []
    return [p3.Table(air, p3.to_mont(t.astype(np.uint64)), (), prep=base.prep)]


SHAPES = {"mix": lambda s: K.mix_tables(6, seed=s), "demo": lambda s: p3.lookup_demo_tables_prep(6, 4, seed=s), "gate": _gate_shard}


@pytest.fixture(scope="module")
def ctx():
    R.p2_tables(1)
    h = H.HipHal(0)
    blob = h.set_params(1, **FAST)
    yield h, blob
    h.close()


@pytest.fixture(scope="module")
def runs(ctx):
    """per shape: the five shards, their key and the single-context proofs (computed once, shared, never changed)"""
    hal, _blob = ctx
    out = {}
    for name, make in SHAPES.items():
        shards = [(make(s), _init(s)) for s in range(N_SHARDS)]
        for tables, _i in shards[1:]:       # one preprocessed matrix per table across the shards, different traces
            for a, b in zip(tables, shards[0][0]):
                assert (a.prep is None and b.prep is None) or np.array_equal(a.prep, b.prep)
        assert not np.array_equal(shards[0][0][0].trace, shards[1][0][0].trace)
        key = p3.setup(hal, shards[0][0])
        out[name] = (shards, key, [p3.prove(hal, t, i, key=key) for t, i in shards])
    yield out
    for _s, key, _w in out.values():
        key.close()


@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_pool_proofs_are_the_single_context_words(ctx, runs, shape, batch):
    hal, blob = ctx
    shards, key, want = runs[shape]
    got = p3.prove_shards(shards, blob, batch=batch, verify=True, key=key)
    assert len(got) == N_SHARDS
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (shape, batch, k)
    assert len({pf.tobytes() for pf in got}) == N_SHARDS
    if batch == 2:
        tables, init = shards[3]
        RP.check_proof(1, BLOW, tables, init, got[3], key.root, queries=FAST["queries"])
        assert p3.verify(K.pinned(tables), got[3], init, params=blob, prep_root=key.root) == 0


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_host_and_device_traces_in_one_run(ctx, runs, shape):
    hal, blob = ctx
    shards, key, want = runs[shape]
    bufs = [hal.copy_from_elem(t.trace) for t in shards[1][0]]
    try:
        hal.sync()
        dev = [None, [(b.ptr, t.log_height) for b, t in zip(bufs, shards[1][0])]] + [None] * (N_SHARDS - 2)
        got = p3.prove_shards(shards, blob, batch=2, verify=True, key=key, device_traces=dev)
    finally:
        for b in bufs:
            b.free()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def test_broken_shard_is_named(ctx, runs):
    """a trace that breaks a constraint through a preprocessed column: the proof is made, the keyed verifier refuses it"""
    hal, blob = ctx
    shards, key, _want = runs["gate"]
    bad = list(shards)
    bad[3] = ([K.break_gate(shards[3][0][0], row=2)], shards[3][1])
    with pytest.raises(_lib.RkError) as e:
        p3.prove_shards(bad, blob, batch=2, verify=True, key=key)
    assert e.value.status == _lib.RK_ERR_VERIFY and e.value.segment == 3
    # without verification the pool returns the (false) proof, which the keyed verifier refuses with reason 3
    pf = p3.prove_shards(bad, blob, batch=2, verify=False, key=key)[3]
    assert p3.verify(K.pinned(bad[3][0]), pf, bad[3][1], params=blob, prep_root=key.root) == 3


def _raw_call(shards, blob, keys, fill=0xDEADBEEF):
    """rk_p3_prove_shards_key / rk_p3_prove_shards (keys None) with proof buffers holding a fill pattern -> (status,
    failed index, the buffers)"""
    lib = _lib.load()
    n = len(shards)
    arr = (_lib.RkP3Shard * n)()
    keep, bufs = [], []
    for i, (tables, init) in enumerate(shards):
        ctab, k = p3._c_tables(tables)
        iw = np.ascontiguousarray(init, dtype=np.uint32)
        buf = np.full(1 << 16, fill, dtype=np.uint32)
        arr[i].tables, arr[i].n_tables = ctab, len(tables)
        arr[i].init_words, arr[i].n_init = iw.ctypes.data_as(_lib.u32p), iw.size
        arr[i].h_proof, arr[i].capacity_words = buf.ctypes.data_as(_lib.u32p), buf.size
        keep += [ctab, k, iw]
        bufs.append(buf)
    opts = _lib.RkP3SessionOpts(device=0, batch=2, verify=1, params=C.pointer(blob))
    failed = C.c_size_t(0)
    if keys is None:
        st = lib.rk_p3_prove_shards(C.byref(opts), arr, n, C.byref(failed))
    else:
        karr = (C.c_void_p * len(keys))(*[None if k is None else k._handle.value for k in keys])
        st = lib.rk_p3_prove_shards_key(C.byref(opts), karr, arr, n, C.byref(failed))
    del keep
    return st, failed.value, bufs


NONE = C.c_size_t(-1).value


def test_refusals_leave_the_buffers_untouched(ctx, runs):
    hal, blob = ctx
    shards, key, _want = runs["gate"]
    untouched = lambda bufs: all((b == 0xDEADBEEF).all() for b in bufs)
    # tables with preprocessed columns and no key: rk_p3_prove_shards keeps refusing
    st, failed, bufs = _raw_call(shards, blob, None)
    assert st == _lib.RK_ERR_INVALID and failed == 0 and untouched(bufs)
    # a NULL entry
    st, failed, bufs = _raw_call(shards, blob, [None])
    assert st == _lib.RK_ERR_INVALID and untouched(bufs)
    # a key over other heights / another prep_width / another table count: the shard at fault is named
    for other in ([K.gate_table(4, 5, True)], [K.gate_table(3, 1)], K.mix_tables(6)):
        k2 = p3.setup(hal, other)
        try:
            st, failed, bufs = _raw_call(shards, blob, [k2])
            assert st == _lib.RK_ERR_INVALID and failed == 0 and untouched(bufs)
        finally:
            k2.close()
    # one shard of another height among fitting ones
    mixed = list(shards)
    mixed[2] = ([K.gate_table(4, 5, True)], shards[2][1])
    st, failed, bufs = _raw_call(mixed, blob, [key])
    assert st == _lib.RK_ERR_INVALID and failed == 2 and untouched(bufs)
    # a key from another parameter set (another blow-up: other LDEs, another tree)
    h2 = H.HipHal(0)
    try:
        h2.set_params(1, blowup_log2=2, **FAST)
        k3 = p3.setup(h2, [K.gate_table(3, 5, True, seed=4, air=K.gate_air(5, True))])
        try:
            st, failed, bufs = _raw_call(shards, blob, [k3])
            assert st == _lib.RK_ERR_INVALID and failed == NONE and untouched(bufs)
        finally:
            k3.close()
    finally:
        h2.close()
    # NOT exercised here: a key of another device than its slot's and keys with different roots -- both need a second GPU
    # (a second device number is refused by the device check before the keys are looked at)
    # an empty batch is RK_OK whatever the keys
    lib = _lib.load()
    opts = _lib.RkP3SessionOpts(device=0, batch=2, verify=1, params=C.pointer(blob))
    assert lib.rk_p3_prove_shards_key(C.byref(opts), None, None, 0, None) == 0     # nothing to prove
    # and the fitting key still proves
    st, failed, bufs = _raw_call(shards[:1], blob, [key])
    assert st == 0 and failed == NONE and not untouched(bufs)


def test_key_without_preprocessed_columns_gives_the_plain_pool_words(ctx):
    hal, blob = ctx
    shards = [(p3.lookup_demo_tables(5, 3, seed=s), _init(s)) for s in range(3)]
    key = p3.setup(hal, shards[0][0])
    try:
        assert key.root is None
        want = p3.prove_shards(shards, blob, batch=2, verify=True)
        got = p3.prove_shards(shards, blob, batch=2, verify=True, key=key)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
    finally:
        key.close()
