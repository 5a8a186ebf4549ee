"""TEST INFRASTRUCTURE: an exact reference for what a uni-stark proof (rk_p3_prove / or_p3_prove) opens, in plain Python
integers and numpy uint64 -- nothing of the oracle or of the product is called, the proof words are only read.

Everything is restated from Plonky3's definitions (p3-uni-stark prover.rs / verifier.rs / folder.rs, p3-commit
domain.rs, p3-challenger duplex_challenger.rs, RECALLED):

* `transcript`: a DuplexChallenger over the plain Poseidon2 of tests/p2_edges.py (`permute`, canonical cells).  observe
  clears the output buffer and absorbs into the input buffer, permuting when it holds `rate` cells (the state's first
  cells are overwritten); sample permutes when input is pending or no output is left, and pops the LAST output cell;
  an extension element is four samples, component 0 first.  Order: the init words; the trace root, every table's public
  values; [with interactions: the two permutation challenges, the permutation root, the cumulative sums]; alpha; the
  quotient root; zeta.
* `trace_openings`: each trace column interpolated over H_n (the subgroup of order n = 2^k, generator g = root(k)) and
  evaluated at zeta and zeta * g.
* `quotient_chunks`: the constraints evaluated on the disjoint coset s * H_(n qd) (x_i = s * w^i, w = root(k + lqd));
  the local row is the trace interpolants at x_i, the next row those at x_i * g = x_(i + qd); selectors
  is_first_row = Z_H(x) / (x - 1), is_last_row = Z_H(x) / (x - g^-1), is_transition = x - g^-1, Z_H(x) = x^n - 1;
  folded acc = acc * alpha + c over the asserts in order, divided by Z_H(x).  split_evals: chunk j takes the points
  j, j + qd, ... -- i.e. the values on the coset D_j = s w^j H_n; each chunk is flattened to its four base components,
  every component interpolated over D_j and evaluated at zeta.
* `recombine`: quotient(zeta) = sum_j zps_j * sum_e x^e chunk_j[e](zeta), zps_j = prod_(i != j) Z_(D_i)(zeta) /
  Z_(D_i)(first point of D_j), Z_(D_i)(y) = (y / (s w^i))^n - 1; for a trace that satisfies its AIR this equals
  fold(zeta) / Z_H(zeta), with the fold taken over the opened trace values.
"""
import numpy as np

import field_ref as F
import p2_edges as E
from raiko_amd import p3

P = F.P
# preset -> (W of x^4 - W, generator of the 2^27 subgroup, coset shift, Poseidon2 width, m4)
PRESETS = {0: (F.W_RISC0, F.GEN_RISC0, 3, 24, 0), 1: (F.W_SP1, F.GEN_SP1, 31, 16, 1)}
_P2_TABLES = {}


def p2_tables(preset):
    """(ext, internal, diag) of the preset's Poseidon2 as canonical integers (the constants, read once)"""
    w, m4 = PRESETS[preset][3:]
    if (w, m4) not in _P2_TABLES:
        _P2_TABLES[(w, m4)] = E.preset_tables(w, m4)
    return _P2_TABLES[(w, m4)]


# ---------------------------------------------------------------- exact linear algebra mod p
def matmod(a, b):
    """a @ b mod p for canonical uint64 matrices, inner dimension <= 2^12: b split into 16-bit limbs so that no partial
    sum leaves uint64 (2^31 * 2^16 * 2^12 < 2^64)"""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    assert a.shape[-1] <= 1 << 12
    lo = (a @ (b & np.uint64(0xFFFF))) % np.uint64(P)
    hi = (a @ (b >> np.uint64(16))) % np.uint64(P)
    return (lo + hi * np.uint64(1 << 16)) % np.uint64(P)


def powers(x, n):
    """x^0 .. x^(n-1) of a base-field x"""
    out = np.ones(n, dtype=np.uint64)
    have, xb = 1, x % P
    while have < n:
        m = min(have, n - have)
        out[have:have + m] = F.vmul(out[:m], xb)
        xb = xb * xb % P
        have += m
    return out


def interpolate(values, k, gen):
    """natural coefficients (n, m) of the columns of `values` (n, m), read as evaluations at g^i, g = root(k)"""
    n = 1 << k
    idx = np.arange(n, dtype=np.uint64)
    winv = powers(F.inv(F.root(k, gen)), n)
    return F.vmul(matmod(winv[np.outer(idx, idx) % n], values), F.inv(n))


def eval_base_poly_at(coeffs, z, W):
    """(m, 4): the extension values at z of the m columns of base coefficients (n, m)"""
    pw = F.ext_powers(z, coeffs.shape[0], W)
    return matmod(np.ascontiguousarray(pw.T), coeffs).T


# ---------------------------------------------------------------- transcript
class Challenger:
    def __init__(self, preset):
        self.width, self.m4 = PRESETS[preset][3:]
        self.tabs = p2_tables(preset)
        self.rate = self.width - 8
        self.state, self.inp, self.out = [0] * self.width, [], []

    def _duplex(self):
        for i, v in enumerate(self.inp):
            self.state[i] = v
        self.inp = []
        self.state = E.permute(self.state, self.m4, *self.tabs)
        self.out = list(self.state[: self.rate])

    def observe(self, vals):
        for v in vals:
            self.out = []
            self.inp.append(int(v) % P)
            if len(self.inp) == self.rate:
                self._duplex()

    def sample(self):
        if self.inp or not self.out:
            self._duplex()
        return self.out.pop()

    def sample_ext(self):
        return tuple(self.sample() for _ in range(4))


def parse(tables, words):
    """the proof's head (n_tables | log_height.. | roots | cumulative sums | opened values); field elements canonical"""
    raw = [int(v) for v in words]
    nt = raw[0]                          # the count and the heights are plain integers, field elements Montgomery words
    assert nt == len(tables)
    out = {"log_n": raw[1:1 + nt]}
    w = [int(v) for v in F.from_mont(np.asarray(words, dtype=np.uint64))]
    pos = 1 + nt

    def take(m):
        nonlocal pos
        pos += m
        return w[pos - m:pos]

    out["trace_root"] = take(8)
    perm = [t for t in tables if t.air.perm_width]
    if perm:
        out["perm_root"] = take(8)
        out["cumsums"] = [take(4) for _ in perm]
    out["quotient_root"] = take(8)
    ext4 = lambda flat: [tuple(flat[4 * c:4 * c + 4]) for c in range(len(flat) // 4)]
    out["tables"] = []
    for t in tables:
        wd, pw, qd = t.air.width, t.air.perm_width, 1 << t.air.log_quotient_degree()
        o = {"local": ext4(take(4 * wd)), "next": ext4(take(4 * wd))}
        if pw:
            o["perm_local"], o["perm_next"] = ext4(take(4 * pw)), ext4(take(4 * pw))
        o["chunks"] = [ext4(take(16)) for _ in range(qd)]
        out["tables"].append(o)
    return out


def transcript(preset, tables, init_canonical, pf):
    """-> (alpha, zeta, (perm alpha, perm beta) or None) replayed from the proof's roots"""
    ch = Challenger(preset)
    ch.observe(init_canonical)
    ch.observe(pf["trace_root"])
    for t in tables:
        ch.observe(F.from_mont(t.public_values))
    pch = None
    if "perm_root" in pf:
        pch = (ch.sample_ext(), ch.sample_ext())
        ch.observe(pf["perm_root"])
        for c in pf["cumsums"]:
            ch.observe(c)
    alpha = ch.sample_ext()
    ch.observe(pf["quotient_root"])
    return alpha, ch.sample_ext(), pch


# ---------------------------------------------------------------- the AIR over extension arrays
def eval_steps(air, local, nxt, public, sel, alpha, W):
    """folded constraints: local / nxt (m, width, 4), public canonical, sel = (is_first, is_last, is_trans) (m, 4) each;
    -> (m, 4).  Main-trace AIRs only."""
    m = local.shape[0]
    embed = lambda v: np.broadcast_to(np.array([v % P, 0, 0, 0], dtype=np.uint64), (m, 4))
    vals, acc = [], np.zeros((m, 4), dtype=np.uint64)
    a4 = np.array(alpha, dtype=np.uint64)
    for op, a, b in air.steps.tolist():
        if op == p3.CONST:
            vals.append(embed(a))
        elif op == p3.LOCAL:
            vals.append(local[:, a])
        elif op == p3.NEXT:
            vals.append(nxt[:, a])
        elif op == p3.PUBLIC:
            vals.append(embed(int(public[a])))
        elif op in (p3.IS_FIRST_ROW, p3.IS_LAST_ROW, p3.IS_TRANSITION):
            vals.append(sel[op - p3.IS_FIRST_ROW])
        elif op == p3.ADD:
            vals.append(F.vadd(vals[a], vals[b]))
        elif op == p3.SUB:
            vals.append(F.vsub(vals[a], vals[b]))
        elif op == p3.MUL:
            vals.append(F.vext_mul(vals[a], vals[b], W))
        elif op == p3.NEG:
            vals.append(F.vsub(0, vals[a]))
        elif op == p3.ASSERT_ZERO:
            acc = F.vadd(F.vext_mul(acc, a4, W), vals[a])
        else:
            raise ValueError("eval_steps: permutation leaves are not covered (op %d)" % op)
    return acc


def _embed_cols(v):
    """(m, w) base -> (m, w, 4)"""
    out = np.zeros(v.shape + (4,), dtype=np.uint64)
    out[..., 0] = v
    return out


# ---------------------------------------------------------------- the checks
def trace_openings(table, zeta, preset):
    """(local, next): the trace interpolants at zeta and zeta * g_n, lists of extension tuples"""
    W, gen = PRESETS[preset][:2]
    k = table.log_height
    C = interpolate(F.from_mont(table.trace), k, gen)
    zn = F.ext_scale(zeta, F.root(k, gen))
    rows = lambda z: [tuple(int(c) for c in r) for r in eval_base_poly_at(C, z, W)]
    return rows(zeta), rows(zn)


def quotient_chunks(table, alpha, zeta, preset, blowup_log2):
    """[chunk j: 4 extension tuples (one per base component)] of the exact quotient"""
    W, gen, s = PRESETS[preset][:3]
    air, k = table.air, table.log_height
    lqd = air.log_quotient_degree()
    assert lqd <= blowup_log2
    n, qd = 1 << k, 1 << lqd
    nq = n << lqd
    C = interpolate(F.from_mont(table.trace), k, gen)
    pq = powers(F.root(k + lqd, gen), nq)
    i, j = np.arange(nq, dtype=np.uint64), np.arange(n, dtype=np.uint64)
    xs = F.vmul(pq, s)
    A = F.vmul(pq[np.outer(i, j) % nq], powers(s, n)[None, :])          # A[i, j] = x_i^j
    local = matmod(A, C)
    nxt = np.roll(local, -qd, axis=0)                                      # x_i * g = x_(i + qd)
    zh = F.vsub(F.vmul(pq[(i * n) % nq], pow(s, n, P)), 1)
    g_inv = F.inv(F.root(k, gen))
    sel = [F.vmul(zh, F.batch_inv(F.vsub(xs, 1))), F.vmul(zh, F.batch_inv(F.vsub(xs, g_inv))), F.vsub(xs, g_inv)]
    acc = eval_steps(air, _embed_cols(local), _embed_cols(nxt), F.from_mont(table.public_values),
                     [_embed_cols(v) for v in sel], alpha, W)
    q = F.vext_scale(acc, F.batch_inv(zh))
    out = []
    for c in range(qd):
        a = s * pow(F.root(k + lqd, gen), c, P) % P                       # D_c = a * H_n
        D = interpolate(q[c::qd], k, gen)                                   # q_c(a * g^r) as a polynomial in g^r
        out.append([tuple(int(v) for v in r) for r in eval_base_poly_at(D, F.ext_scale(zeta, F.inv(a)), W)])
    return out


def recombine(chunks, zeta, log_n, lqd, preset):
    """sum_j zps_j * sum_e x^e chunk_j[e]"""
    W, gen, s = PRESETS[preset][:3]
    n, qd, w = 1 << log_n, 1 << lqd, F.root(log_n + lqd, gen)
    shifts = [s * pow(w, j, P) % P for j in range(qd)]
    tot = (0, 0, 0, 0)
    for j in range(qd):
        zp = (1, 0, 0, 0)
        for i in range(qd):
            if i != j:
                num = F.ext_sub(F.ext_pow(F.ext_scale(zeta, F.inv(shifts[i])), n, W), (1, 0, 0, 0))
                den = (pow(shifts[j] * F.inv(shifts[i]) % P, n, P) - 1) % P
                zp = F.ext_mul(zp, F.ext_scale(num, F.inv(den)), W)
        for e in range(4):
            mono = tuple(int(t == e) for t in range(4))
            tot = F.ext_add(tot, F.ext_mul(F.ext_mul(zp, mono, W), chunks[j][e], W))
    return tot


def folded_at_zeta(table, local, nxt, alpha, zeta, preset):
    """fold(zeta) / Z_H(zeta) over opened rows"""
    W, gen = PRESETS[preset][:2]
    n = 1 << table.log_height
    one = (1, 0, 0, 0)
    zh = F.ext_sub(F.ext_pow(zeta, n, W), one)
    g_inv = F.inv(F.root(table.log_height, gen))
    zg = F.ext_sub(zeta, (g_inv, 0, 0, 0))
    sel = [F.ext_mul(zh, F.ext_inv(F.ext_sub(zeta, one), W), W), F.ext_mul(zh, F.ext_inv(zg, W), W), zg]
    arr = lambda rows: np.array([rows], dtype=np.uint64)
    acc = eval_steps(table.air, arr(local), arr(nxt), F.from_mont(table.public_values),
                     [np.array([v], dtype=np.uint64) for v in sel], alpha, W)
    return F.ext_mul(tuple(int(v) for v in acc[0]), F.ext_inv(zh, W), W)


def check_proof(preset, blowup_log2, tables, init_mont, words, quotient=True):
    """every check above on one proof; raises AssertionError naming what differs.  quotient=False (or a table with
    interactions): the trace openings only.  -> (alpha, zeta)"""
    pf = parse(tables, words)
    assert pf["log_n"] == [t.log_height for t in tables]
    alpha, zeta, _ = transcript(preset, tables, F.from_mont(np.asarray(init_mont, dtype=np.uint64)), pf)
    for ti, (t, op) in enumerate(zip(tables, pf["tables"])):
        loc, nxt = trace_openings(t, zeta, preset)
        assert op["local"] == loc, "table %d: trace_local" % ti
        assert op["next"] == nxt, "table %d: trace_next" % ti
        if not quotient or t.air.perm_width:
            continue
        lqd = t.air.log_quotient_degree()
        want = quotient_chunks(t, alpha, zeta, preset, blowup_log2)
        for j, (got, exp) in enumerate(zip(op["chunks"], want)):
            assert got == exp, "table %d: quotient chunk %d of %d" % (ti, j, 1 << lqd)
        assert recombine(want, zeta, t.log_height, lqd, preset) == folded_at_zeta(t, loc, nxt, alpha, zeta, preset), \
            "table %d: zps recombination" % ti
    return alpha, zeta
