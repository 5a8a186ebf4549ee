"""Exact reference arithmetic for the BabyBear kernels, in plain Python integers and numpy uint64.

Independent of both C implementations (the oracle under oracle/ and the product): every value here comes from
the definitions -- p = 15 * 2^27 + 1, the quartic extension Fp[x]/(x^4 - W), roots of unity taken from a generator of
the 2^27 subgroup -- and numpy is only used to vectorise the same modular operations.  Element values are
canonical integers in [0, p); `to_mont` / `from_mont` convert to and from the Montgomery words (R = 2^32) that the
device buffers hold.

NTT conventions (the risc0 ones the kernels follow):
  interpolate: natural-order evaluations x_i = f(w^i) -> coefficients c_j of f, stored at position bitrev_k(j);
  evaluate:    coefficients at bit-reversed positions -> natural-order evaluations;
  expand (e):  n coefficients at bitrev_k positions -> the 2^e n evaluations f(w_{2^e n}^i);
  zk_shift:    the word at position q is multiplied by shift^bitrev_k(q) (coefficient j by shift^j).
Closed forms for structured inputs (`*_impulse`, `*_constant`, `*_alternating`, `*_monomial`) cost O(n) vectorised
operations, so they serve the largest transform (2^24 points) in about a second.
"""
import numpy as np

P = 2013265921
R = 1 << 32
RINV = pow(R, -1, P)
W_RISC0 = P - 11     # x^4 + 11
W_SP1 = 11           # x^4 - 11
GEN_RISC0 = 137      # generates the 2^27 subgroup (risc0, the kernels' default tables)
GEN_SP1 = 0x1A427A41
TWO_ADICITY = 27


# ---------------------------------------------------------------- base field
def to_mont(x):
    """canonical -> Montgomery word; int or array"""
    if isinstance(x, (int, np.integer)):
        return int(x) % P * R % P
    return (np.asarray(x, dtype=np.uint64) % P * (R % P) % P).astype(np.uint32)


def from_mont(x):
    if isinstance(x, (int, np.integer)):
        return int(x) * RINV % P
    return (np.asarray(x, dtype=np.uint64) * RINV % P).astype(np.uint64)


def inv(a: int) -> int:
    a %= P
    if a == 0:
        raise ZeroDivisionError("0 has no inverse")
    return pow(a, P - 2, P)


def vmul(a, b):
    """elementwise product of canonical uint64 arrays (products < 2^62)"""
    return np.asarray(a, dtype=np.uint64) * np.asarray(b, dtype=np.uint64) % P


def vadd(a, b):
    return (np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64)) % P


def vsub(a, b):
    return (np.asarray(a, dtype=np.uint64) + P - np.asarray(b, dtype=np.uint64)) % P


def vpow(base: int, exps) -> np.ndarray:
    """base^e for an array of exponents 0 <= e < 2^32, through two 2^16-entry tables"""
    e = np.asarray(exps, dtype=np.uint64)
    lo = np.empty(1 << 16, dtype=np.uint64)
    hi = np.empty(1 << 16, dtype=np.uint64)
    cur = 1
    for i in range(1 << 16):
        lo[i] = cur
        cur = cur * base % P
    step, cur = cur, 1   # base^(2^16)
    for i in range(1 << 16):
        hi[i] = cur
        cur = cur * step % P
    return vmul(hi[(e >> 16) & 0xFFFF], lo[e & 0xFFFF])


def batch_inv(a) -> np.ndarray:
    """elementwise inverse of a nonzero array: a product tree, one scalar inversion, and the tree back down"""
    a = np.asarray(a, dtype=np.uint64)
    n = a.size
    if n == 0:
        return a.copy()
    m = 1 << (n - 1).bit_length()
    levels = [np.concatenate([a, np.ones(m - n, dtype=np.uint64)])]
    while levels[-1].size > 1:
        t = levels[-1]
        levels.append(vmul(t[0::2], t[1::2]))
    cur = np.array([inv(int(levels[-1][0]))], dtype=np.uint64)
    for t in reversed(levels[:-1]):
        nxt = np.empty(t.size, dtype=np.uint64)
        nxt[0::2] = vmul(cur, t[1::2])
        nxt[1::2] = vmul(cur, t[0::2])
        cur = nxt
    return cur[:n]


# ---------------------------------------------------------------- quartic extension Fp[x]/(x^4 - W)
def ext(v):
    """an int or a 4-sequence -> tuple of 4 canonical ints"""
    if isinstance(v, (int, np.integer)):
        return (int(v) % P, 0, 0, 0)
    return tuple(int(c) % P for c in v)


def ext_add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def ext_sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def ext_scale(a, s: int):
    return tuple(x * s % P for x in a)


def ext_mul(a, b, W=W_RISC0):
    r = [0] * 7
    for i in range(4):
        for j in range(4):
            r[i + j] += a[i] * b[j]
    return tuple((r[i] + W * r[i + 4]) % P if i < 3 else r[3] % P for i in range(4))


def ext_pow(a, e: int, W=W_RISC0):
    r, b = (1, 0, 0, 0), a
    while e:
        if e & 1:
            r = ext_mul(r, b, W)
        b = ext_mul(b, b, W)
        e >>= 1
    return r


def ext_inv(a, W=W_RISC0):
    if not any(a):
        raise ZeroDivisionError("0 has no inverse")
    return ext_pow(a, P ** 4 - 2, W)


def ext_to_mont(a) -> np.ndarray:
    return np.array([to_mont(int(c)) for c in a], dtype=np.uint32)


def ext_from_mont(words):
    return tuple(from_mont(int(c)) for c in words)


def vext_mul(a, b, W=W_RISC0):
    """elementwise product of (..., 4) canonical arrays"""
    a = np.asarray(a, dtype=np.uint64)
    b = np.asarray(b, dtype=np.uint64)
    r = [np.zeros(np.broadcast_shapes(a.shape[:-1], b.shape[:-1]), dtype=np.uint64) for _ in range(7)]
    for i in range(4):
        for j in range(4):
            r[i + j] = vadd(r[i + j], vmul(a[..., i], b[..., j]))
    out = [vadd(r[i], vmul(r[i + 4], W)) for i in range(3)] + [r[3]]
    return np.stack(out, axis=-1)


def vext_scale(a, s):
    """(..., 4) extension array times a (...) base-field array"""
    return vmul(np.asarray(a, dtype=np.uint64), np.asarray(s, dtype=np.uint64)[..., None])


# ---------------------------------------------------------------- roots of unity and orderings
def root(k: int, gen: int = GEN_RISC0) -> int:
    """the 2^k-th root of unity the transforms use: gen^(2^(27-k))"""
    return pow(gen, 1 << (TWO_ADICITY - k), P)


def bitrev(i: int, bits: int) -> int:
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def bitrev_perm(bits: int) -> np.ndarray:
    """r[i] = bitrev_bits(i) for i < 2^bits"""
    r = np.zeros(1, dtype=np.uint64)
    for _ in range(bits):
        r = np.concatenate([2 * r, 2 * r + 1])
    return r


# ---------------------------------------------------------------- O(n^2) DFT, n <= 2^10
def dft_evaluate(coeffs_natural, N: int, gen: int = GEN_RISC0, shift: int = 1):
    """f(shift * w_N^i), i < N, for natural-order coefficients"""
    k = N.bit_length() - 1
    w = root(k, gen)
    c = [int(x) for x in coeffs_natural]
    out = []
    for i in range(N):
        x = shift * pow(w, i, P) % P
        acc = 0
        for cj in reversed(c):
            acc = (acc * x + cj) % P
        out.append(acc)
    return out


def dft_interpolate(evals, gen: int = GEN_RISC0):
    """natural-order coefficients of the polynomial with f(w^i) = evals[i]"""
    n = len(evals)
    k = n.bit_length() - 1
    winv = inv(root(k, gen))
    ninv = inv(n)
    x = [int(v) for v in evals]
    return [sum(x[i] * pow(winv, i * j, P) for i in range(n)) * ninv % P for j in range(n)]


def to_bitrev_order(natural):
    k = len(natural).bit_length() - 1
    return [natural[bitrev(p, k)] for p in range(len(natural))]


def ntt_interpolate(evals, gen=GEN_RISC0):
    """what batch_interpolate_ntt leaves: coefficients at bit-reversed positions"""
    return to_bitrev_order(dft_interpolate(evals, gen))


def ntt_evaluate(coeffs_bitrev, expand_bits: int = 0, gen=GEN_RISC0):
    """what batch_evaluate_ntt (expand_bits = 0) or batch_expand_into_evaluate_ntt leaves"""
    nat = to_bitrev_order(list(coeffs_bitrev))
    return dft_evaluate(nat, len(nat) << expand_bits, gen)


def zk_shift(words_bitrev, shift: int = 3):
    k = len(words_bitrev).bit_length() - 1
    return [int(v) * pow(shift, bitrev(q, k), P) % P for q, v in enumerate(words_bitrev)]


# ---------------------------------------------------------------- closed forms, any n up to 2^24
def geom(x, m: int) -> np.ndarray:
    """sum_{j < m} x^j, elementwise over an array of x"""
    x = np.asarray(x, dtype=np.uint64)
    out = np.full(x.shape, m % P, dtype=np.uint64)
    ne = x != 1
    if ne.any():
        xm = np.array([pow(int(v), m, P) for v in x[ne]], dtype=np.uint64) if x[ne].size < 64 else None
        if xm is None:
            raise ValueError("geom: use geom_roots for long arrays")
        out[ne] = vmul(vsub(1, xm), batch_inv(vsub(1, x[ne])))
    return out


def geom_roots(k: int, m: int, gen: int = GEN_RISC0) -> np.ndarray:
    """sum_{j < m} (w^i)^j for every i < 2^k, w = root(k); m a power of two <= 2^k"""
    n = 1 << k
    i = np.arange(n, dtype=np.uint64)
    x = vpow(root(k, gen), i)
    xm = vpow(root(k, gen), (i * m) % n)
    out = np.full(n, m % P, dtype=np.uint64)
    ne = x != 1
    out[ne] = vmul(vsub(1, xm[ne]), batch_inv(vsub(1, x[ne])))
    return out


def evaluate_impulse(k: int, q: int, v: int, expand_bits: int = 0, gen=GEN_RISC0) -> np.ndarray:
    """evaluate / expand of a column whose only nonzero word v sits at position q: the coefficient of x^j,
    j = bitrev_k(q), so output i is v * w_N^(i j)"""
    N = 1 << (k + expand_bits)
    j = bitrev(q, k)
    i = np.arange(N, dtype=np.uint64)
    return vmul(vpow(root(k + expand_bits, gen), (i * j) % N), v)


def evaluate_constant(k: int, v: int, expand_bits: int = 0, gen=GEN_RISC0) -> np.ndarray:
    """every coefficient c_0 .. c_(n-1) equal to v: output i = v * sum_{j < n} w_N^(i j)"""
    return vmul(geom_roots(k + expand_bits, 1 << k, gen), v)


def evaluate_alternating(k: int, v: int, expand_bits: int = 0, gen=GEN_RISC0) -> np.ndarray:
    """v at odd positions, 0 at even: the odd positions hold coefficients n/2 .. n-1, so output i is
    v * w_N^(i n/2) * sum_{j < n/2} w_N^(i j)"""
    N = 1 << (k + expand_bits)
    half = 1 << (k - 1)
    i = np.arange(N, dtype=np.uint64)
    return vmul(vmul(vpow(root(k + expand_bits, gen), (i * half) % N), geom_roots(k + expand_bits, half, gen)), v)


def interpolate_impulse(k: int, q: int, v: int, gen=GEN_RISC0) -> np.ndarray:
    """evaluations v at natural index q, 0 elsewhere: c_j = v/n * w^-(q j), stored at bitrev_k(j)"""
    n = 1 << k
    j = bitrev_perm(k)
    return vmul(vpow(inv(root(k, gen)), (j * q) % n), v * inv(n) % P)


def interpolate_constant(k: int, v: int) -> np.ndarray:
    out = np.zeros(1 << k, dtype=np.uint64)
    out[0] = v % P
    return out


def interpolate_alternating(k: int, v: int) -> np.ndarray:
    """v at odd natural indices: v (1 - (-1)^i) / 2 = v/2 - v/2 w^(i n/2), coefficients 0 and n/2 (positions 0 and 1)"""
    out = np.zeros(1 << k, dtype=np.uint64)
    h = v * inv(2) % P
    out[0] = h
    out[1] = (P - h) % P
    return out


def interpolate_monomial(k: int, m: int, v: int, gen=GEN_RISC0):
    """(evaluations v * w^(i m), the interpolation: v at position bitrev_k(m))"""
    n = 1 << k
    ev = vmul(vpow(root(k, gen), (np.arange(n, dtype=np.uint64) * m) % n), v)
    out = np.zeros(n, dtype=np.uint64)
    out[bitrev(m, k)] = v % P
    return ev, out


def zk_shift_vec(words_bitrev, shift: int = 3) -> np.ndarray:
    """zk_shift of a whole column at any size"""
    w = np.asarray(words_bitrev, dtype=np.uint64)
    k = w.size.bit_length() - 1
    return vmul(w, vpow(shift, bitrev_perm(k)))


# ---------------------------------------------------------------- polynomial steps (extension coefficients)
def horner(coeffs, x, W=W_RISC0):
    """sum_i coeffs[i] x^i, extension coefficients and point"""
    acc = (0, 0, 0, 0)
    for c in reversed(list(coeffs)):
        acc = ext_add(ext_mul(acc, x, W), c)
    return acc


def vhorner_base(coeffs, x, W=W_RISC0):
    """f(x) for base-field coefficients (array) at an extension point: sum c_i x^i via a table of powers"""
    pw = ext_powers(x, len(coeffs), W)
    return tuple(int(v) for v in (vmul(pw, np.asarray(coeffs, dtype=np.uint64)[:, None]).sum(axis=0) % P))


def ext_powers(x, n: int, W=W_RISC0) -> np.ndarray:
    """(n, 4) array of x^0 .. x^(n-1), by doubling blocks: x^(b + i) = x^b * x^i"""
    out = np.zeros((n, 4), dtype=np.uint64)
    if n == 0:
        return out
    out[0] = (1, 0, 0, 0)
    have, xb = 1, np.array(x, dtype=np.uint64)
    while have < n:
        m = min(have, n - have)
        out[have:have + m] = vext_mul(out[:m], xb, W)
        xb = vext_mul(xb, xb, W)
        have += m
    return out


def poly_divide(coeffs, z, W=W_RISC0):
    """synthetic division by (x - z): (quotient[n] with quotient[n-1] = 0, remainder f(z)), as risc0's poly_divide
    leaves it: q_(i-1) = c_i + z q_i from the top, in place"""
    c = [ext(v) for v in coeffs]
    n = len(c)
    q = [(0, 0, 0, 0)] * n
    cur = (0, 0, 0, 0)
    for i in range(n - 1, -1, -1):
        nxt = ext_add(ext_mul(z, cur, W), c[i])
        q[i] = cur
        cur = nxt
    return q, cur


def vpoly_divide(coeffs, z, W=W_RISC0):
    """poly_divide on an (n, 4) array in O(n) vectorised steps for a base-field z (the Horner chain is linear:
    q_(i-1) = sum_{t >= i} c_t z^(t - i), a suffix sum of c_t z^t scaled by z^-i), falls back to the loop otherwise"""
    c = np.asarray(coeffs, dtype=np.uint64)
    z = ext(z)
    if not any(z):                   # division by x: the quotient is the shifted coefficients, the remainder c_0
        q = np.zeros_like(c)
        q[:-1] = c[1:]
        return q, tuple(int(v) for v in c[0])
    if any(z[1:]):
        q, r = poly_divide(c.tolist(), z, W)
        return np.array(q, dtype=np.uint64), r
    n = c.shape[0]
    zp = vpow(z[0], np.arange(n, dtype=np.uint64))
    zi = vpow(inv(z[0]), np.arange(n, dtype=np.uint64))
    t = vmul(c, zp[:, None])
    # suffix sums of t (exact: object dtype would be slow; reduce blocks of 2^20 terms < 2^51)
    suf = np.zeros_like(t)
    run = np.zeros(4, dtype=np.uint64)
    B = 1 << 20
    for s in range((n - 1) // B * B, -1, -B):
        blk = t[s:s + B]
        cs = np.flip(np.cumsum(np.flip(blk, axis=0), axis=0), axis=0) % P
        suf[s:s + B] = (cs + run) % P
        run = suf[s].copy()
    rem = tuple(int(v) for v in suf[0])
    q = np.zeros_like(c)
    q[:-1] = vmul(suf[1:], zi[1:, None])   # q_(i-1) = z^-i * sum_{t >= i} c_t z^t
    return q, rem


def poly_multiply_linear(coeffs, z, W=W_RISC0):
    """coeffs(x) * (x - z): a polynomial with a root at z"""
    c = [ext(v) for v in coeffs]
    out = [(0, 0, 0, 0)] * (len(c) + 1)
    for i, v in enumerate(c):
        out[i + 1] = ext_add(out[i + 1], v)
        out[i] = ext_sub(out[i], ext_mul(z, v, W))
    return out


def prefix_products(elems, W=W_RISC0):
    out, cur = [], (1, 0, 0, 0)
    for e in elems:
        cur = ext_mul(cur, ext(e), W)
        out.append(cur)
    return out


def mix_sum(out0, mix_start, mix, columns, combos, W=W_RISC0):
    """mix_poly_coeffs: out[combo[i]][idx] += mix_start * mix^i * columns[i][idx]; out0 (ncombo, count, 4), columns
    (w, count) canonical arrays"""
    out = np.array(out0, dtype=np.uint64)
    cur = ext(mix_start)
    for i in range(len(combos)):
        out[combos[i]] = vadd(out[combos[i]], vext_scale(np.array(cur, dtype=np.uint64), columns[i]))
        cur = ext_mul(cur, ext(mix), W)
    return out


def fri_fold(planes, out_count: int, mix, log_a: int, W=W_RISC0) -> np.ndarray:
    """risc0 fri_fold: planes (4, A * out_count), out[idx] = sum_i mix^i f[bitrev(i) * count + idx]; returns (4, count)"""
    A = 1 << log_a
    pl = np.asarray(planes, dtype=np.uint64).reshape(4, A, out_count)
    tot = np.zeros((out_count, 4), dtype=np.uint64)
    cur = (1, 0, 0, 0)
    for i in range(A):
        f = pl[:, bitrev(i, log_a), :].T
        tot = vadd(tot, vext_mul(f, np.array(cur, dtype=np.uint64), W))
        cur = ext_mul(cur, ext(mix), W)
    return tot.T


def fri_fold_evals(evals, beta, W=W_SP1, gen=GEN_SP1) -> np.ndarray:
    """Plonky3's arity-2 fold on bit-reversed evaluations over the subgroup of order 2 n_out: (2 n_out, 4) ->
    (n_out, 4), out[i] = (a + b)/2 + beta (a - b) / (2 x), x = g^bitrev_(k-1)(i)"""
    e = np.asarray(evals, dtype=np.uint64)
    n_out = e.shape[0] // 2
    k = (2 * n_out).bit_length() - 1
    xs = vpow(root(k, gen), bitrev_perm(k - 1)) if k > 1 else np.ones(1, dtype=np.uint64)
    half = inv(2)
    a, b = e[0::2], e[1::2]
    even = vmul(vadd(a, b), half)
    odd = vext_scale(vsub(a, b), vmul(batch_inv(xs), half))
    return vadd(even, vext_mul(odd, np.array(ext(beta), dtype=np.uint64), W))


# ---------------------------------------------------------------- Plonky3 PCS steps
def coset_lde_natural(evals_col, blowup_log2: int, shift: int, gen: int):
    """evaluations over the subgroup of order h -> values at shift * w_(h 2^b)^j, j natural (O(n^2))"""
    c = dft_interpolate(evals_col, gen)
    c = [v * pow(shift, i, P) % P for i, v in enumerate(c)]
    return dft_evaluate(c, len(c) << blowup_log2, gen)


def pcs_eval_at(lde_rows, H: int, blowup_log2: int, z, shift: int, gen: int, W: int):
    """opened values p_c(z) of a row-major LDE (rows at bit-reversed coset positions): interpolate the low coset
    (its value at shift * g^i sits in row bitrev_k(i), g = root(k)) exactly and evaluate at z; O(h^2) unless the
    column is constant"""
    kb = H.bit_length() - 1
    k = kb - blowup_log2
    h = 1 << k
    lde = np.asarray(lde_rows, dtype=np.uint64).reshape(H, -1)
    w = lde.shape[1]
    # low coset: x_i = shift * g^i, g = root(k); its value sits at row bitrev_k(i)
    perm = bitrev_perm(k)
    sinv = inv(shift)
    out = []
    for c in range(w):
        ys = lde[perm, c]
        if (ys == ys[0]).all():      # the interpolant of a constant column is that constant
            out.append(ext(int(ys[0])))
            continue
        # coefficients of p(shift x) from values at g^i, then p(z) = sum a_j (z / shift)^j
        a = dft_interpolate([int(v) for v in ys], gen)
        zz = ext_scale(z, sinv)
        out.append(horner([ext(v) for v in a], zz, W))
    return out


def pcs_reduce_openings(ro, lde_rows, H: int, points, ys, alpha, alpha_offset: int, shift: int, gen: int, W: int):
    """ro[r] += alpha^(offset + j w) (sum_c alpha^c M[r][c] - sum_c alpha^c y_j[c]) / (x_r - z_j),
    x_r = shift * w_H^bitrev(r); vectorised over rows"""
    kb = H.bit_length() - 1
    lde = np.asarray(lde_rows, dtype=np.uint64).reshape(H, -1)
    w = lde.shape[1]
    apow = ext_powers(ext(alpha), w, W)
    rr = np.zeros((H, 4), dtype=np.uint64)
    for c in range(w):
        rr = vadd(rr, vext_scale(np.broadcast_to(apow[c], (H, 4)), lde[:, c]))
    xs = vmul(vpow(root(kb, gen), bitrev_perm(kb)), shift)
    out = np.array(ro, dtype=np.uint64).reshape(H, 4)
    for j, z in enumerate(points):
        z = ext(z)
        rys = (0, 0, 0, 0)
        for c in range(w):
            rys = ext_add(rys, ext_mul(tuple(int(v) for v in apow[c]), ext(ys[j][c]), W))
        off = ext_pow(ext(alpha), alpha_offset + j * w, W)
        num = vext_mul(vsub(rr, np.array(rys, dtype=np.uint64)), np.array(off, dtype=np.uint64), W)
        den = np.zeros((H, 4), dtype=np.uint64)
        den[:, 0] = vsub(xs, z[0])
        for t in (1, 2, 3):
            den[:, t] = (P - z[t]) % P
        out = vadd(out, vext_mul(num, vext_inv_many(den, W), W))
    return out


def vext_inv_many(a, W=W_RISC0) -> np.ndarray:
    """elementwise inverse of a nonzero (n, 4) extension array via the norm to Fp[y]/(y^2 - W), y = x^2
    (a closed formula of the field's algebra, checked against ext_inv in tests/test_field_ref.py)"""
    a = np.asarray(a, dtype=np.uint64)
    c0, c1, c2, c3 = (a[:, i] for i in range(4))
    # a = A0 + A1 x, A0 = c0 + c2 y, A1 = c1 + c3 y; a (A0 - A1 x) = A0^2 - y A1^2 = n0 + n1 y
    n0 = vsub(vadd(vmul(c0, c0), vmul(W, vmul(c2, c2))), vmul(W, vmul(2, vmul(c1, c3))))
    n1 = vsub(vsub(vmul(2, vmul(c0, c2)), vmul(c1, c1)), vmul(W, vmul(c3, c3)))
    d = vsub(vmul(n0, n0), vmul(W, vmul(n1, n1)))
    di = batch_inv(d)
    m0, m1 = vmul(n0, di), vsub(0, vmul(n1, di))
    conj = np.stack([c0, vsub(0, c1), c2, vsub(0, c3)], axis=-1)
    m = np.stack([m0, np.zeros_like(m0), m1, np.zeros_like(m0)], axis=-1)
    return vext_mul(conj, m, W)
