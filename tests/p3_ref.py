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

Tables with interactions (sp1-core's LogUp argument: lookup/interaction.rs, stark/permutation.rs, RECALLED; the
constraints are the ones raiko_amd/p3.py::_perm_constraints states):

* `perm_trace`: per interaction rlc = alpha + bus + sum_j beta^(j+1) x_j and the term +-mult / rlc (send +, receive -);
  entry b of a row = the terms of interactions 2b and 2b + 1; the last extension column is the inclusive running sum of
  the rows' totals.  The cumulative sum is its last row.
* the leaves of `eval_steps`: PERM_LOCAL / PERM_NEXT a = base column a of the permutation trace (embedded on the
  quotient coset, an extension value where it is opened), CHALLENGE a = word a of [alpha | 1 | beta | beta^2 ..],
  CUMSUM a = word a of the table's cumulative sum.
* `open_columns_at`: the O(n) barycentric opening f(z) = (z^n - 1) / n * sum_i f_i g^i / (z - g^i), for tables too
  tall for the dense `interpolate` (which stays, and cross-checks it at small k).
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


def open_columns_at(values, k, z, preset):
    """[extension tuple per column]: the interpolants over H_n (n = 2^k) of the canonical base columns `values` (n, m)
    at the extension point z outside H_n, by the barycentric formula f(z) = (z^n - 1) / n * sum_i f_i g^i / (z - g^i):
    O(n) per column, one vext_inv_many per point"""
    W, gen = PRESETS[preset][:2]
    n = 1 << k
    values = np.asarray(values, dtype=np.uint64).reshape(n, -1)
    gi = powers(F.root(k, gen), n)
    den = np.empty((n, 4), dtype=np.uint64)
    den[:, 0] = F.vsub(int(z[0]) % P, gi)
    den[:, 1:] = np.array([int(c) % P for c in z[1:]], dtype=np.uint64)
    wgt = F.vext_scale(F.vext_inv_many(den, W), gi)                       # g^i / (z - g^i)
    acc = np.zeros((values.shape[1], 4), dtype=np.uint64)
    for at in range(0, n, 1 << 12):                                          # matmod's inner dimension stays <= 2^12
        acc = F.vadd(acc, matmod(np.ascontiguousarray(values[at:at + (1 << 12)].T), wgt[at:at + (1 << 12)]))
    scale = F.ext_scale(F.ext_sub(F.ext_pow(tuple(int(c) for c in z), n, W), (1, 0, 0, 0)), F.inv(n))
    return [tuple(int(c) for c in r) for r in F.vext_mul(acc, np.array(scale, dtype=np.uint64), W)]


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
def eval_steps(air, local, nxt, public, sel, alpha, W, perm=None):
    """folded constraints: local / nxt (m, width, 4), public canonical, sel = (is_first, is_last, is_trans) (m, 4) each;
    perm (AIRs with interactions) = (permutation local (m, perm_width, 4), next, challenge words, cumulative sum words);
    -> (m, 4)"""
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
        elif op == p3.PERM_LOCAL:
            vals.append(perm[0][:, a])
        elif op == p3.PERM_NEXT:
            vals.append(perm[1][:, a])
        elif op == p3.CHALLENGE:
            vals.append(embed(int(perm[2][a])))
        elif op == p3.CUMSUM:
            vals.append(embed(int(perm[3][a])))
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
            raise ValueError("eval_steps: no such opcode (%d)" % op)
    return acc


def _embed_cols(v):
    """(m, w) base -> (m, w, 4)"""
    out = np.zeros(v.shape + (4,), dtype=np.uint64)
    out[..., 0] = v
    return out


# ---------------------------------------------------------------- the permutation (LogUp) argument
MAX_VALUES = 64      # the longest tuple an interaction may hold


def challenge_words(pch, W, n_values=MAX_VALUES):
    """[alpha | 1 | beta | beta^2 .. beta^n_values] as canonical base words: what a CHALLENGE leaf indexes"""
    alpha, beta = pch
    out, cur = [int(c) for c in alpha], (1, 0, 0, 0)
    for _ in range(n_values + 1):
        out += [int(c) for c in cur]
        cur = F.ext_mul(cur, tuple(int(c) for c in beta), W)
    return out


def perm_entries(trace, interactions, chal, W):
    """(entries (n, nb, 4), row totals (n, 4)) of a canonical main trace (n, width): term i = +-mult_i / rlc_i,
    rlc_i = chal[0] + chal[1] bus + sum_j chal[2 + j] x_j over the extension elements chal[e] = words 4e .. 4e + 3 (send +,
    receive -, mult a constant or a column); entry b = terms 2b and 2b + 1; total = the sum of a row's entries"""
    trace = np.asarray(trace, dtype=np.uint64)
    n = trace.shape[0]
    ch = np.array([int(c) for c in chal], dtype=np.uint64).reshape(-1, 4)
    nb = (len(interactions) + 1) // 2
    entries = np.zeros((n, nb, 4), dtype=np.uint64)
    for i, it in enumerate(interactions):
        rlc = np.broadcast_to(F.vadd(ch[0], F.vmul(ch[1], it.bus % P)), (n, 4))
        for j, c in enumerate(it.value_cols):
            rlc = F.vadd(rlc, F.vext_scale(ch[2 + j], trace[:, c]))
        m = np.full(n, it.mult % P, dtype=np.uint64) if it.mult_is_const else trace[:, it.mult]
        if it.kind == p3.RECEIVE:
            m = F.vsub(0, m)
        entries[:, i // 2] = F.vadd(entries[:, i // 2], F.vext_scale(F.vext_inv_many(rlc, W), m))
    return entries, entries.sum(axis=1) % np.uint64(P)                    # nb <= 2^11 terms below 2^31 each


def perm_trace(table, pch, preset):
    """the permutation trace of a table with interactions under the challenges pch = (alpha, beta): canonical uint64
    (n, 4 (nb + 1)), nb = ceil(L / 2): the nb batch entries, then the inclusive running sum of the row totals"""
    W = PRESETS[preset][0]
    its = table.air.interactions
    assert its and table.log_height <= 32 and len(its) <= 4096
    entries, totals = perm_entries(F.from_mont(table.trace), its, challenge_words(pch, W, max(len(it.value_cols) for it in its)), W)
    n = totals.shape[0]
    phi = np.cumsum(totals, axis=0) % np.uint64(P)                        # canonical terms: below 2^(31 + log_n) <= 2^63
    return np.concatenate([entries.reshape(n, -1), phi], axis=1)


# ---------------------------------------------------------------- the checks
def openings(values, k, zeta, preset, tall=False):
    """(at zeta, at zeta * g_n) of canonical base columns (n, m), lists of extension tuples: the dense interpolation, or
    the O(n) form when tall"""
    W, gen = PRESETS[preset][:2]
    zn = F.ext_scale(zeta, F.root(k, gen))
    if tall:
        return open_columns_at(values, k, zeta, preset), open_columns_at(values, k, zn, preset)
    C = interpolate(values, k, gen)
    rows = lambda z: [tuple(int(c) for c in r) for r in eval_base_poly_at(C, z, W)]
    return rows(zeta), rows(zn)


def trace_openings(table, zeta, preset, tall=False):
    """(local, next): the trace interpolants at zeta and zeta * g_n, lists of extension tuples"""
    return openings(F.from_mont(table.trace), table.log_height, zeta, preset, tall)


def quotient_chunks(table, alpha, zeta, preset, blowup_log2, perm=None):
    """[chunk j: 4 extension tuples (one per base component)] of the exact quotient.  perm (a table with interactions) =
    (its permutation trace (n, perm_width) canonical, challenge words, cumulative sum words): on the quotient coset the
    permutation rows are the interpolants of that trace's base columns, the next row (cyclically) those at x * g"""
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
    pv = None
    if perm is not None:
        pl = matmod(A, interpolate(perm[0], k, gen))
        pv = (_embed_cols(pl), _embed_cols(np.roll(pl, -qd, axis=0)), perm[1], perm[2])
    acc = eval_steps(air, _embed_cols(local), _embed_cols(nxt), F.from_mont(table.public_values),
                     [_embed_cols(v) for v in sel], alpha, W, pv)
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


def folded_at_zeta(table, local, nxt, alpha, zeta, preset, perm=None):
    """fold(zeta) / Z_H(zeta) over opened rows.  perm = (opened perm_local, opened perm_next, challenge words, cumulative
    sum words) for a table with interactions"""
    W, gen = PRESETS[preset][:2]
    n = 1 << table.log_height
    one = (1, 0, 0, 0)
    zh = F.ext_sub(F.ext_pow(zeta, n, W), one)
    g_inv = F.inv(F.root(table.log_height, gen))
    zg = F.ext_sub(zeta, (g_inv, 0, 0, 0))
    sel = [F.ext_mul(zh, F.ext_inv(F.ext_sub(zeta, one), W), W), F.ext_mul(zh, F.ext_inv(zg, W), W), zg]
    arr = lambda rows: np.array([rows], dtype=np.uint64)
    pv = None if perm is None else (arr(perm[0]), arr(perm[1]), perm[2], perm[3])
    acc = eval_steps(table.air, arr(local), arr(nxt), F.from_mont(table.public_values),
                     [np.array([v], dtype=np.uint64) for v in sel], alpha, W, pv)
    return F.ext_mul(tuple(int(v) for v in acc[0]), F.ext_inv(zh, W), W)


def check_proof(preset, blowup_log2, tables, init_mont, words, quotient=True, tall=False, perm_out=None):
    """every check above on one proof; raises AssertionError naming what differs.  Tables with interactions: the
    cumulative sum, then the permutation openings in every base column, and their quotient like any other table's.
    quotient=False: no quotient chunks.  tall=True (tables too tall for the dense matrices): every opening by the O(n)
    formula and no quotient; the transcript, trace openings, cumulative sums and permutation openings are still checked.
    perm_out: a dict that receives {table index: the reference permutation trace}.  -> (alpha, zeta)"""
    W = PRESETS[preset][0]
    pf = parse(tables, words)
    assert pf["log_n"] == [t.log_height for t in tables]
    alpha, zeta, pch = transcript(preset, tables, F.from_mont(np.asarray(init_mont, dtype=np.uint64)), pf)
    # the cumulative sums first: they depend on the permutation challenges alone, every later challenge depends on them
    ptraces, chal = {}, None
    if pch is not None:
        chal = challenge_words(pch, W)
        for pi, ti in enumerate(i for i, t in enumerate(tables) if t.air.perm_width):
            ptraces[ti] = perm_trace(tables[ti], pch, preset)
            assert ptraces[ti].shape[1] == tables[ti].air.perm_width
            assert pf["cumsums"][pi] == [int(v) for v in ptraces[ti][-1, -4:]], "table %d: cumulative sum" % ti
        if perm_out is not None:
            perm_out.update(ptraces)
    for ti, (t, op) in enumerate(zip(tables, pf["tables"])):
        loc, nxt = trace_openings(t, zeta, preset, tall)
        assert op["local"] == loc, "table %d: trace_local" % ti
        assert op["next"] == nxt, "table %d: trace_next" % ti
        perm_q = perm_z = None
        if t.air.perm_width:
            ploc, pnxt = openings(ptraces[ti], t.log_height, zeta, preset, tall)
            for what, got, exp in (("perm_local", op["perm_local"], ploc), ("perm_next", op["perm_next"], pnxt)):
                assert len(got) == len(exp) == t.air.perm_width
                for c, (g, e) in enumerate(zip(got, exp)):
                    assert g == e, "table %d: %s column %d of %d" % (ti, what, c, t.air.perm_width)
            cs = [int(v) for v in ptraces[ti][-1, -4:]]
            perm_q, perm_z = (ptraces[ti], chal, cs), (ploc, pnxt, chal, cs)
        if not quotient or tall:
            continue
        lqd = t.air.log_quotient_degree()
        want = quotient_chunks(t, alpha, zeta, preset, blowup_log2, perm_q)
        for j, (got, exp) in enumerate(zip(op["chunks"], want)):
            assert got == exp, "table %d: quotient chunk %d of %d" % (ti, j, 1 << lqd)
        assert recombine(want, zeta, t.log_height, lqd, preset) == folded_at_zeta(t, loc, nxt, alpha, zeta, preset, perm_z), \
            "table %d: zps recombination" % ti
    return alpha, zeta
