"""Preprocessed columns on the GPU: rk_p3_setup / rk_p3_prove_key / rk_p3_verify_key against the exact reference of
tests/p3_ref_prep.py (integers and numpy; nothing of the product is called by it), at the shapes where the new code can
go wrong -- the fourth column group of the quotient evaluator (interpreter, and the hiprtc-generated kernel for two
AIRs), the preprocessed rows in perm_entries_kernel, the preprocessed batch in the opening round, in the reduced openings
and in the queries (a tree of its own height).

Every shape: the proof's words against the reference (transcript with the root observed, all openings, cumulative sums,
quotient chunks, recombination, total length), rk_p3_verify_key = 0 against the key's root, a proof made under a key over
a preprocessed matrix with one cell changed refused against the honest root, and a trace that breaks a constraint through
a preprocessed column refused with reason 3."""
import ctypes as C

import numpy as np
import pytest

import p3_prep_cases as K
import p3_ref as R
import p3_ref_prep as RP
from raiko_amd import _lib, hal as H, p3

pytestmark = pytest.mark.gpu
OVER = dict(queries=3, pow_bits=1)
BLOW = 1          # the SP1 preset's blow-up
INIT = p3.to_mont([20241, 7])


@pytest.fixture(scope="module")
def ctx():
    R.p2_tables(1)
    h = H.HipHal(0)
    blob = h.set_params(1, **OVER)
    yield h, blob
    h.close()


def _judge(ctx, tables, breaker=None, changed=None, compile_airs=False):
    """the four checks of a shape; breaker = (table index, function giving the broken table), changed = the table index
    whose preprocessed matrix gets one cell changed (default: the first with preprocessed columns)"""
    hal, blob = ctx
    key = p3.setup(hal, tables)
    try:
        pf = p3.prove(hal, tables, INIT, key=key)
        RP.check_proof(1, BLOW, tables, INIT, pf, key.root, queries=OVER["queries"])
        ver = K.pinned(tables)
        assert p3.verify(ver, pf, INIT, params=blob, prep_root=key.root) == 0
        if compile_airs:                                   # the generated kernel gives the interpreter's words
            for t in tables:
                t.air.compile(hal)
            assert np.array_equal(p3.prove(hal, tables, INIT, key=key), pf), "generated kernel against interpreter"
        ti = changed if changed is not None else next(i for i, t in enumerate(tables) if t.air.prep_width)
        forged = list(tables)
        forged[ti] = K.with_prep_cell_changed(tables[ti], row=1)
        bad_key = p3.setup(hal, forged)
        try:
            assert not np.array_equal(bad_key.root, key.root)
            bad = p3.prove(hal, tables, INIT, key=bad_key)
            assert p3.verify(ver, bad, INIT, params=blob, prep_root=key.root) != 0
            assert p3.verify(ver, bad, INIT, params=blob, prep_root=bad_key.root) in (0, 3, 8)   # consistent with ITS key, if at all
        finally:
            bad_key.close()
        if breaker is not None:
            bi, fn = breaker
            broken = list(tables)
            broken[bi] = fn(tables[bi])
            bpf = p3.prove(hal, broken, INIT, key=key)
            assert p3.verify(ver, bpf, INIT, params=blob, prep_root=key.root) == 3
        return pf, key.root.copy()
    finally:
        key.close()


@pytest.mark.parametrize("log_n,cw,cubic", [(1, 1, False), (1, 5, True), (3, 1, True), (3, 5, False), (6, 1, False), (6, 5, True)])
def test_gate_air_heights_and_widths(ctx, log_n, cw, cubic):
    """log_height 1, 3, 6 x prep_width 1, 5; PREP_NEXT across the wrap-around row under is_transition in every one, the
    degree-3 constraint prep . local . local (two quotient chunks) in half of them.  At 2 rows the next row of row 1 is
    row 0: the smallest wrap"""
    t = K.gate_table(log_n, cw, cubic)
    assert t.air.log_quotient_degree() == (1 if cubic else 0)
    _judge(ctx, [t], breaker=(0, lambda tb: K.break_gate(tb, row=(1 << log_n) - 1)))


def test_generated_kernel_reads_the_fourth_group(ctx):
    """hiprtc for two AIRs: the cubic gate (PREP_LOCAL and PREP_NEXT taps, stride 0 at two chunks) and the mixed lookup
    sender (permutation AND preprocessed taps in one kernel)"""
    t = K.gate_table(4, 5, True, seed=3)
    _judge(ctx, [t], breaker=(0, K.break_gate), compile_airs=True)
    hal, blob = ctx
    tables = K.mix_tables(6, seed=2)
    key = p3.setup(hal, tables)
    try:
        pf = p3.prove(hal, tables, INIT, key=key)
        tables[0].air.compile(hal)
        assert np.array_equal(p3.prove(hal, tables, INIT, key=key), pf)
        RP.check_proof(1, BLOW, tables, INIT, pf, key.root, queries=OVER["queries"])
    finally:
        key.close()


def test_only_the_middle_table_has_preprocessed_columns(ctx):
    tables = [p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(4)), K.gate_table(3, 5, True, seed=1),
              p3.Table.from_canonical(p3.cubic_air(6), *p3.cubic_trace(5, 6, seed=2))]
    _judge(ctx, tables, breaker=(1, K.break_gate))


def test_preprocessed_table_shortest_and_tallest(ctx):
    """shortest: the preprocessed tree is lower than the trace tree (its query index loses the low bits, its path is
    shorter); tallest: it has the global maximum height while the other tables' rows repeat"""
    fib = lambda k: p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(k))
    _judge(ctx, [fib(6), K.gate_table(3, 1)], breaker=(1, K.break_gate))
    _judge(ctx, [fib(2), K.gate_table(6, 5)], breaker=(1, K.break_gate))


def test_lookups_over_main_and_preprocessed_columns(ctx):
    """a tuple mixing a main and a preprocessed column, a multiplicity that is a preprocessed column, a receiver whose
    tuple is preprocessed altogether; 64 and 512 sender rows (less than one perm_entries workgroup, and two).  A changed
    preprocessed multiplicity unbalances the sums; a changed w breaks w = v * k"""
    for log_n in (6, 9):
        tables = K.mix_tables(log_n)

        def brk(tb):
            t = p3.from_mont(tb.trace).astype(np.uint64)
            t[3, 1] = (t[3, 1] + 1) % K.P
            return p3.Table.from_canonical(tb.air, t, (), prep=p3.from_mont(tb.prep))
        _judge(ctx, tables, breaker=(0, brk))


@pytest.mark.parametrize("log_cpu", [4, 10])
def test_range_prep_demo(ctx, log_cpu):
    """the cpu / add / mul tables of lookup_demo_tables looking up into the preprocessed range table (log_range 4)"""
    hal, blob = ctx
    tables = p3.lookup_demo_tables_prep(log_cpu, 4, seed=log_cpu)
    assert tables[3].air.prep_width == 1 and tables[3].air.width == 1 and tables[3].air.n_constraints == 16
    pf, root = _judge(ctx, tables, changed=3)
    # a multiplicity off by one: the sums no longer cancel
    t = p3.from_mont(tables[3].trace).astype(np.uint64)
    t[0, 0] = (t[0, 0] + 1) % K.P
    off = tables[:3] + [p3.Table.from_canonical(tables[3].air, t, (), prep=p3.from_mont(tables[3].prep))]
    key = p3.setup(hal, tables)
    try:
        assert np.array_equal(key.root, root)              # the same matrix, the same root
        assert p3.verify(K.pinned(tables), p3.prove(hal, off, INIT, key=key), INIT, params=blob, prep_root=root) == 8
    finally:
        key.close()


def test_one_key_three_proofs(ctx):
    hal, blob = ctx
    air = K.gate_air(5, True)
    base = K.gate_table(5, 5, True, seed=4, air=air)
    key = p3.setup(hal, [base])
    try:
        root = key.root.copy()
        s = p3.from_mont(base.prep).astype(object)
        proofs = []
        for x0 in (1, 2, 3):                                # three main traces over the one preprocessed matrix
            t = np.zeros((32, 3), dtype=object)
            x = x0
            for r in range(32):
                y = (int(s[r][0]) * x + sum(int(v) for v in s[r][1:])) % K.P
                t[r] = [x, y, int(s[r][0]) * x * y % K.P]
                x = (x + int(s[(r + 1) % 32][4])) % K.P
            tb = p3.Table(air, p3.to_mont(t.astype(np.uint64)), (), prep=base.prep)
            pf = p3.prove(hal, [tb], INIT, key=key)
            RP.check_proof(1, BLOW, [tb], INIT, pf, root, queries=OVER["queries"])
            assert p3.verify(K.pinned([tb]), pf, INIT, params=blob, prep_root=root) == 0
            assert np.array_equal(p3.prove(hal, [tb], INIT, key=key), pf)    # the same inputs twice: identical words
            proofs.append(pf)
        assert not np.array_equal(proofs[0], proofs[1])
        back = np.zeros(8, dtype=np.uint32)
        assert _lib.load().rk_p3_key_root(key._handle, back.ctypes.data_as(_lib.u32p)) == 0
        assert np.array_equal(back, root)
        assert key.bytes >= (64 * 5 + 32 * 0 + 2 * 64 * 8) * 4
    finally:
        key.close()


def test_empty_key_proves_the_bytes_of_rk_p3_prove(ctx):
    hal, blob = ctx
    jobs = [[p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(5))],
            [p3.Table.from_canonical(p3.cubic_air(6), *p3.cubic_trace(6, 6, seed=1))],
            p3.lookup_demo_tables(5, 3, seed=1)]
    for tables in jobs:
        key = p3.setup(hal, tables)
        try:
            assert key.root is None and key.bytes == 0
            want = p3.prove(hal, tables, INIT)
            assert np.array_equal(p3.prove(hal, tables, INIT, key=key), want)
            assert p3.verify(tables, want, INIT, params=blob) == 0
        finally:
            key.close()


def test_refusals(ctx):
    hal, blob = ctx
    lib = _lib.load()
    t = K.gate_table(3, 1)
    with pytest.raises(_lib.RkError) as e:
        p3.prove(hal, [t], INIT)                           # rk_p3_prove on a prep AIR (its bound is 0: nothing to size)
    assert e.value.status == _lib.RK_ERR_INVALID
    arr, keep = p3._c_tables([t])
    out, n = np.zeros(1 << 16, dtype=np.uint32), C.c_size_t(0)
    iw = np.ascontiguousarray(INIT)
    assert lib.rk_p3_prove(hal._ctx, arr, 1, iw.ctypes.data_as(_lib.u32p), iw.size, out.ctypes.data_as(_lib.u32p), out.size, C.byref(n)) == _lib.RK_ERR_INVALID
    assert lib.rk_p3_prove_key(hal._ctx, None, arr, 1, iw.ctypes.data_as(_lib.u32p), iw.size, out.ctypes.data_as(_lib.u32p), out.size, C.byref(n)) == _lib.RK_ERR_INVALID
    key = p3.setup(hal, [t])
    try:
        pf = p3.prove(hal, [t], INIT, key=key)
        for other in ([K.gate_table(4, 1)], [K.gate_table(3, 5)], [t, t],
                      [p3.Table.from_canonical(p3.fibonacci_air(), *p3.fibonacci_trace(3))]):   # a key from another shape
            with pytest.raises(_lib.RkError) as e:
                p3.prove(hal, other, INIT, key=key)
            assert e.value.status == _lib.RK_ERR_INVALID
        ver = K.pinned([t])
        assert p3.verify(ver, pf, INIT, params=blob) == _lib.RK_ERR_INVALID                  # rk_p3_verify on a prep AIR
        with pytest.raises(_lib.RkError) as e:
            p3.verify_hashes(ver, pf, INIT, params=blob)
        assert e.value.status == _lib.RK_ERR_INVALID
        varr, vkeep = p3._c_tables(ver)
        shape, w = (C.c_uint32 * 4)(), [C.c_size_t(0) for _ in range(3)]
        pw, buf = pf.ctypes.data_as(_lib.u32p), np.zeros(1 << 20, dtype=np.uint32)
        bp, cap = buf.ctypes.data_as(_lib.u32p), 1 << 18
        ip = iw.ctypes.data_as(_lib.u32p)
        assert lib.rk_p3_fri_openings(C.byref(blob), varr, 1, ip, iw.size, pw, pf.size, shape, bp, cap, bp, cap, C.byref(w[0]), C.byref(w[1])) == _lib.RK_ERR_INVALID
        assert lib.rk_p3_fri_inputs(C.byref(blob), varr, 1, ip, iw.size, pw, pf.size, shape, bp, cap, bp, cap, bp, cap, C.byref(w[0]), C.byref(w[1]),
                                    C.byref(w[2])) == _lib.RK_ERR_INVALID
        assert lib.rk_p3_fri_input_paths(C.byref(blob), varr, 1, ip, iw.size, pw, pf.size, shape, bp, cap, bp, cap, C.byref(w[0]), C.byref(w[1])) == _lib.RK_ERR_INVALID
        assert lib.rk_p3_fri_transcript(C.byref(blob), varr, 1, ip, iw.size, pw, pf.size, shape, bp, cap, bp, cap, bp, cap, C.byref(w[0]), C.byref(w[1]),
                                        C.byref(w[2])) == _lib.RK_ERR_INVALID
        with pytest.raises(_lib.RkError) as e:
            p3.prove_shards([([t], INIT)], blob)
        assert e.value.status == _lib.RK_ERR_INVALID
        del keep, vkeep
    finally:
        key.close()
