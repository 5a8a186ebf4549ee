"""TEST INFRASTRUCTURE: the AIRs and tables the preprocessed-column tests share (tests/test_p3_prep.py on the CPU,
tests/test_gpu_p3_prep.py on the GPU, tools/make_p3_prep_golden.py for the committed fixtures).

gate_air(cw, cubic): main columns (x, y, z), cw preprocessed columns s_0 .. s_(cw-1):
    y = s_0 * x + s_1 + .. + s_(cw-1)                                   PREP_LOCAL of every column, degree 2
    is_transition * (next x - x - next s_(cw-1)) = 0                    PREP_NEXT; on the last row next s is ROW 0's (the
                                                                        wrap-around), which only is_transition excuses
    cubic: z = s_0 * x * y                                              prep . local . local: degree 3, two quotient chunks
    otherwise z is free
mix_tables(log_n): a sender with main (v, w) and preprocessed (k, m) that sends the tuple (v, k) -- a main and a
    preprocessed column mixed -- m times, the multiplicity itself a PREPROCESSED column, and also constrains w = v * k;
    a receiver whose tuple columns (v, k) are both preprocessed and whose multiplicity is its only main column.
"""
import numpy as np

from raiko_amd import p3

P = p3.P
BUS_MIX = 9


def gate_air(cw, cubic=False):
    b = p3.AirBuilder(3, 0, prep_width=cw)
    x, y, z = b.local(0), b.local(1), b.local(2)
    acc = b.prep_local(0) * x
    for c in range(1, cw):
        acc = acc + b.prep_local(c)
    b.assert_eq(y, acc)
    b.when_transition().assert_zero(b.next(0) - x - b.prep_next(cw - 1))
    if cubic:
        b.assert_eq(z, b.prep_local(0) * x * y)
    return b.build()


def gate_table(log_n, cw, cubic=False, seed=0, air=None):
    """-> Table with canonical-consistent trace and preprocessed matrix (both random but for the constraints)"""
    n = 1 << log_n
    g = np.random.default_rng(1000 * log_n + 10 * cw + seed)
    s = g.integers(0, P, size=(n, cw)).astype(object)
    t = np.zeros((n, 3), dtype=object)
    x = int(g.integers(0, P))
    for r in range(n):
        y = (int(s[r][0]) * x + sum(int(v) for v in s[r][1:])) % P
        t[r] = [x, y, int(s[r][0]) * x * y % P if cubic else int(g.integers(0, P))]
        x = (x + int(s[(r + 1) % n][cw - 1])) % P
    air = air or gate_air(cw, cubic)
    assert air.check_trace(t, (), prep=s) == []
    return p3.Table.from_canonical(air, t.astype(np.uint64), (), prep=s.astype(np.uint64))


def break_gate(table, row=0):
    """the same table with y of one row off by one: the constraint y = s_0 x + .. through the preprocessed columns fails"""
    t = p3.from_mont(table.trace).astype(np.uint64)
    t[row % t.shape[0], 1] = (t[row % t.shape[0], 1] + 1) % P
    return p3.Table.from_canonical(table.air, t, (), prep=p3.from_mont(table.prep))


def with_prep_cell_changed(table, row=0, col=0):
    """the same table over a preprocessed matrix with one cell changed (the trace is left alone)"""
    s = p3.from_mont(table.prep).astype(np.uint64)
    s[row % s.shape[0], col] = (s[row % s.shape[0], col] + 1) % P
    return p3.Table(table.air, table.trace, table.public_values, prep=p3.to_mont(s))


def mix_airs():
    snd = p3.AirBuilder(2, 0, prep_width=2)
    snd.assert_eq(snd.local(1), snd.local(0) * snd.prep_local(0))
    snd.send(BUS_MIX, [0, snd.prep(0)], mult=snd.prep(1), mult_is_const=False)
    rcv = p3.AirBuilder(1, 0, prep_width=2)
    rcv.receive(BUS_MIX, [rcv.prep(0), rcv.prep(1)], mult=0, mult_is_const=False)
    return snd.build(), rcv.build()


def mix_tables(log_n, seed=0, airs=None):
    n = 1 << log_n
    r = np.arange(n, dtype=np.uint64)
    g = np.random.default_rng(77 + seed)
    k = r % 4
    m = r % 3                                              # multiplicities 0, 1, 2: a preprocessed column
    v = g.integers(0, 5, size=n).astype(np.uint64)
    snd = np.stack([v, v * k % P], axis=1)
    # the receiver's table: every tuple (v, k) that can occur, fixed before any witness; its counts are the witness
    log_r = 5
    tup = np.zeros((1 << log_r, 2), dtype=np.uint64)
    tup[:20] = [(a, b) for a in range(5) for b in range(4)]
    cnt = np.zeros(1 << log_r, dtype=np.uint64)
    for vi, ki, mi in zip(v.tolist(), k.tolist(), m.tolist()):
        cnt[vi * 4 + ki] += mi
    # the padding rows are the tuple (0, 0) again with count 0: they receive nothing
    sa, ra = airs or mix_airs()
    return [p3.Table.from_canonical(sa, snd, (), prep=np.stack([k, m], axis=1)),
            p3.Table.from_canonical(ra, cnt.reshape(-1, 1), (), prep=tup)]


def pinned(tables):
    """the verifier's tables: no traces, the heights of the tables with preprocessed columns pinned"""
    out = []
    for t in tables:
        v = p3.Table(t.air, None, t.public_values)
        if t.air.prep_width:
            v.log_height = t.log_height
        out.append(v)
    return out
