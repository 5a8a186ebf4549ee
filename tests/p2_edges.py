"""TEST INFRASTRUCTURE: Poseidon2 at the edges of the unreduced arithmetic of poseidon2_core.hpp, for all four shipped
instances (width 24 / 16, external 4x4 block m4 = 0 / 1).

* `permute`: the permutation in plain Python integers, any tables (canonical field values).
* `aim`: round-3 external constants that take a chosen input to a chosen state where the partial rounds begin.
* `ENTRY_SCALE`: what the kernel holds there -- the raw 32-bit cells are centred representatives of the true state
  times 2^(32 e), e = -2800 (the scale schedule of Core::scale_exp), so a target is chosen in that representation.
* `partial_model`: Core::partial_rounds (the blocked form, PR_BLOCK = 3) re-run on Python integers, no wrap, with the
  same order of operations and the same redc64 / fold64 / smul_const, recording the largest magnitude every
  accumulator reaches; the words it multiplies by come from the emulator build of derive() (emul_p2_derived).
* `WORST`: diagonals and internal round constants whose derived words sit at the edge of the centred range
  (found by `search_diag` / `search_rc_int`, kept here as literals so the GPU tests do not repeat the search)."""
import numpy as np

import oracle_lib as o

P = o.P
H = (P - 1) // 2
R1 = (1 << 32) % P
R2 = R1 * R1 % P
INV7 = pow(7, -1, P - 1)
M4 = {0: [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]],
      1: [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]}
INSTANCES = [(24, 0), (24, 1), (16, 0), (16, 1)]          # (width, m4): risc0's, ..., SP1 / Plonky3's
ENTRY_EXP = -2800
ENTRY_SCALE = pow(2, -32 * ENTRY_EXP, P)                  # true entry state = raw representative * ENTRY_SCALE
G = pow(2, 32 * 2801, P)                                  # the first block's factor carried by the block-0 words


def rounds_partial(w):
    return 21 if w == 24 else 13


def m_ext(v, m4):
    w, m = len(v), M4[m4]
    blk = [sum(m[i % 4][j] * v[i - i % 4 + j] for j in range(4)) for i in range(w)]
    tot = [sum(blk[b + j] for b in range(0, w, 4)) for j in range(4)]
    return [(blk[i] + tot[i % 4]) % P for i in range(w)]


def m_ext_matrix(w, m4):
    return [[(2 if i // 4 == j // 4 else 1) * M4[m4][i % 4][j % 4] for j in range(w)] for i in range(w)]


def inverse_mod_p(m):
    n = len(m)
    a = [row[:] + [int(i == j) for j in range(n)] for i, row in enumerate(m)]
    for c in range(n):
        r = next(r for r in range(c, n) if a[r][c] % P)
        a[c], a[r] = a[r], a[c]
        iv = pow(a[c][c], -1, P)
        a[c] = [x * iv % P for x in a[c]]
        for r in range(n):
            if r != c and a[r][c]:
                f = a[r][c]
                a[r] = [(x - f * y) % P for x, y in zip(a[r], a[c])]
    return [row[n:] for row in a]


MINV = {k: inverse_mod_p(m_ext_matrix(*k)) for k in INSTANCES}


def full_round(s, ext, r, m4):
    w = len(s)
    return m_ext([pow((s[i] + ext[r * w + i]) % P, 7, P) for i in range(w)], m4)


def partial_round(s, rc, diag):
    s = list(s)
    s[0] = pow((s[0] + rc) % P, 7, P)
    tot = sum(s)
    return [(tot + d * x) % P for d, x in zip(diag, s)]


def permute(s, m4, ext, internal, diag):
    """Poseidon2, x^7, 4 + R_P + 4 rounds, plain integers; tables canonical, ext flat (8 * W)"""
    s = m_ext([int(x) % P for x in s], m4)
    for r in range(4):
        s = full_round(s, ext, r, m4)
    for rc in internal:
        s = partial_round(s, rc, diag)
    for r in range(4, 8):
        s = full_round(s, ext, r, m4)
    return s


def entry_state(s, m4, ext):
    """the true state where the partial rounds begin"""
    s = m_ext([int(x) % P for x in s], m4)
    for r in range(4):
        s = full_round(s, ext, r, m4)
    return s


def aim(inp, m4, ext, target):
    """ext with its round-3 constants replaced so that `inp` enters the partial rounds as the true state `target`"""
    w = len(inp)
    s = m_ext([int(x) % P for x in inp], m4)
    for r in range(3):
        s = full_round(s, ext, r, m4)
    u = [sum(a * b for a, b in zip(row, target)) % P for row in MINV[(w, m4)]]
    out = list(ext)
    out[3 * w: 4 * w] = [(pow(x, INV7, P) - y) % P for x, y in zip(u, s)]
    return out


def target_of_raw(raw):
    """true entry state whose raw cells are congruent to `raw` (signed representatives)"""
    return [x * ENTRY_SCALE % P for x in raw]


def cen(x):
    x %= P
    return x - P if x > H else x


# ---- entry patterns (raw representatives at the start of the partial rounds) ----
def entry_patterns(w, stream=None):
    """alternating +-h, +-(h - 1), 0 / +-1, a mix, all +h; and, given the derived words, +-h with the sign of the
    block-0 dot-product constant of every cell (so that |D_1| grows with every term) and with the sign of the
    block-0 cell multiplier d_i^3 R G"""
    alt = lambda a: [a if i % 2 == 0 else -a for i in range(w)]
    mix = [H, -H, H - 1, -(H - 1), 0, 1, -1, H + 1]
    pats = {"alt_h": alt(H), "alt_h-1": alt(H - 1), "small": [(0, 1, -1)[i % 3] for i in range(w)],
            "mixed": [mix[i % len(mix)] for i in range(w)], "all_h": [H] * w}
    if stream is not None:
        # block 0: (W - 1) x 2 dot-product words, then per cell d^3 R G, ...
        pats["sign_D1"] = [H] + [H if stream[2 * (i - 1)] >= 0 else -H for i in range(1, w)]
        base = 2 * (w - 1)
        pats["sign_upd"] = [-H] + [H if stream[base + 5 * (i - 1)] >= 0 else -H for i in range(1, w)]
    return pats


# ---- the emulator hooks ----
def mont_tables(ext, internal, diag):
    return [o.to_mont(np.array([int(x) for x in t], dtype=np.uint64)) for t in (ext, internal, diag)]


def emul_entry_cells(emu, w, m4, tabs, inp):
    m = mont_tables(*tabs)
    c = o.to_mont(np.array([int(x) for x in inp], dtype=np.uint64))
    emu.emul_p2_entry_cells(w, m4, o.ptr(m[0]), o.ptr(m[1]), o.ptr(m[2]), o.ptr(c))
    return [int(x) for x in c.view(np.int32)]


def emul_derived(emu, w, m4, tabs):
    """(stream as signed ints, dict of the scalar words)"""
    m = mont_tables(*tabs)
    out = np.zeros(2048, dtype=np.uint32)
    n = emu.emul_p2_derived(w, m4, o.ptr(m[0]), o.ptr(m[1]), o.ptr(m[2]), o.ptr(out))
    v = [int(x) for x in out[: n + 7].view(np.int32)]
    names = ("fix0", "d0", "r2", "r3", "csum0", "csum1", "csum2")
    return v[:n], dict(zip(names, v[n:]))


def emul_permute(emu, w, m4, tabs, inp):
    m = mont_tables(*tabs)
    c = o.to_mont(np.array([int(x) for x in inp], dtype=np.uint64))
    emu.emul_poseidon2_permute_cfg(o.ptr(c), w, m4, o.ptr(m[0]), o.ptr(m[1]), o.ptr(m[2]))
    return [int(x) for x in o.from_mont(c)]


# ---- Core::partial_rounds on Python integers ----
MPRIME = 0x88000001
M32 = (1 << 32) - 1
I64 = 1 << 63

# the bounds poseidon2_core.hpp states for K = 3 (partial_rounds() comment), as (limit, printable)
BOUNDS = {
    "entry": (P / 2 + 53, "p/2 + 53"),
    "X": (0.979 * P, "0.979 p"),
    "y": (0.934 * P, "0.934 p"),
    "D": (2 ** 62.9, "2^62.9"),
    "T": (2 ** 60.5, "2^60.5"),
    "S": (1.37 * H, "1.37 h"),
    "SM2": (1.27 * H, "1.27 h"),
    "x0": (0.88 * P, "0.88 p"),
    "t": (2 ** 61.9, "2^61.9"),
}


class Overflow(AssertionError):
    pass


def _s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def redc64(t):
    if not -I64 <= t < I64:
        raise Overflow("redc64 input outside int64: %d" % t)
    q = _s32((t & M32) * MPRIME)
    u = t - q * P
    assert u & M32 == 0
    r = u >> 32
    if not -(1 << 31) <= r < (1 << 31):
        raise Overflow("redc64 result outside int32: %d" % r)
    return r


def fold64(t):
    if not -I64 <= t < I64:
        raise Overflow("fold64 input outside int64: %d" % t)
    hi = t >> 32
    return t - 2 * hi * P


def canon(r):
    if not -P < r < P:
        raise Overflow("canon input outside (-p, p): %d" % r)
    return r % P


def partial_model(cells, stream, k, rc_int_m, w, block=3):
    """(exit cells, {accumulator: largest |value|}) for raw entry cells `cells` (int32 values), the derived `stream` /
    scalar words `k` (emul_derived) and the internal round constants in Montgomery form"""
    rp = rounds_partial(w)
    nb = (rp + block - 1) // block
    blk_len = lambda b: block if b < rp // block else rp % block
    blk_next = lambda b: blk_len(b + 1) if b + 1 < nb else 1
    nv = w - 1
    peak = {n: 0 for n in BOUNDS}

    def see(name, v):
        if not -I64 <= v < I64:
            raise Overflow("%s outside int64: %d" % (name, v))
        peak[name] = max(peak[name], abs(v))
        return v

    it = iter(stream)
    s = list(cells)
    for x in s:
        see("entry", x)
    x0 = canon(see("x0", redc64(s[0] * k["fix0"])))
    sig = redc64(sum(s[1:])) * k["fix0"]
    csum = [k["csum0"], k["csum1"], k["csum2"]]
    D = {}
    for j in range(1, blk_len(0)):
        D[j] = 0
    for i in range(1, w):
        for j in range(1, blk_len(0)):
            D[j] = see("D", D[j] + next(it) * s[i])
            if i % 4 == 0 and i < nv:
                D[j] = fold64(D[j])
    for b in range(nb):
        kk, kn, r0 = blk_len(b), blk_next(b), b * block
        sp, sm2 = [], 0
        for j in range(kk):
            a = x0 + rc_int_m[r0 + j] - P                      # sbox7_lazy: int32(x + (rc - p))
            assert -(1 << 31) <= a < (1 << 31)
            a2 = redc64(a * a)
            a3 = redc64(a2 * a)
            a6 = redc64(a3 * a3)
            y = see("y", redc64(a6 * a))
            if j == 0:
                T = see("T", sig + y)
            else:
                T = see("T", y + fold64(D[j]))
                for m in range(j):
                    T = see("T", T + sp[m] * csum[j - 1 - m])
            sp.append(see("S", redc64(T)))
            if j + 1 < kk:
                x0 = canon(see("x0", redc64(y * k["d0"] + sp[j] * k["r2"])))
            else:
                sm2 = see("SM2", redc64(sp[j] * k["r3"]))
                x0 = canon(see("x0", redc64(sm2 + y * k["d0"])))
        nsig, nD = 0, {j: 0 for j in range(1, kn)}
        for i in range(1, w):
            t = see("t", sm2 + next(it) * s[i])
            for m in range(kk - 1):
                t = see("t", t + next(it) * sp[m])
            v = see("X", redc64(t))
            s[i] = v
            nsig += v
            for j in range(1, kn):
                nD[j] = see("D", nD[j] + next(it) * v)
                if i % 4 == 0 and i < nv:
                    nD[j] = fold64(nD[j])
        sig, D = nsig, nD
    assert next(it, None) is None, "stream not consumed exactly"
    return [x0] + [canon(x) for x in s[1:]], peak


def margins(peak):
    """{name: limit / largest value seen} (> 1: the stated bound held)"""
    return {n: (BOUNDS[n][0] / peak[n] if peak[n] else float("inf")) for n in BOUNDS}


# ---- aimed constants ----
def diag_words(d, w):
    """the distinct stream words of one cell i >= 1 with true diagonal entry d (numpy uint64 array) and how often each
    occurs in the stream (derive(), PR_BLOCK = 3): block 0's dot products d G, d^2 G and cell update d^3 R G, then per
    block d^3 R, d^2 R^2, d R^2 and the next block's d, d^2; width 16 ends with a one-round block (d R)"""
    d2 = d * d % P
    d3 = d2 * d % P
    nb3 = rounds_partial(w) // 3                            # blocks of three
    words = [(d * G % P, 1), (d2 * G % P, 1), (d3 * R1 % P * G % P, 1), (d3 * R1 % P, nb3 - 1),
             (d2 * R2 % P, nb3), (d * R2 % P, nb3), (d, nb3 - 1), (d2, nb3 - 1)]
    if w == 16:
        words.append((d * R1 % P, 1))
    return words


def edge_count(words):
    """sum of multiplicities of the words whose centred value has |c| >= 0.99 h"""
    tot = 0
    for v, mult in words:
        c = np.where(v > H, P - v, v)
        tot = tot + mult * (c >= int(0.99 * H))
    return tot


def search_diag(w, seed, samples=1 << 21):
    """true diagonal: d_0 with |d_0 R| = h, cells 1 .. W-2 the best-scoring d of a seeded random sample, the last cell
    the best-scoring one that also puts c_1 R = sum_{i >= 1} d_i R at the edge"""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, P, size=samples, dtype=np.uint64)
    sc = edge_count(diag_words(d, w))
    best = sc.max()
    top = d[sc == best]
    top = top[np.argsort(top)]
    first = int(top[0])
    partial = (w - 2) * first
    cand = d[sc >= best - 1]
    c1 = (partial + cand) % P * R1 % P
    c1 = np.where(c1 > H, P - c1, c1)
    order = np.lexsort((cand, -c1, -sc[sc >= best - 1]))
    last = int(cand[order[0]])
    d0 = (H + 1) * pow(R1, -1, P) % P                    # Montgomery form h + 1: centred -h
    return [d0] + [first] * (w - 2) + [last]


def table_score(emu, w, m4, tabs):
    """how many derived words (stream, c_0, c_1) sit at |c| >= 0.99 h, and |d_0|"""
    stream, k = emul_derived(emu, w, m4, tabs)
    words = stream + [k["csum0"], k["csum1"]]
    return sum(abs(c) >= int(0.99 * H) for c in words), abs(k["d0"])


def search_rc_int(w, stream, k, entries, seed, tries):
    """internal round constants that drive the accumulators hardest from the given raw entry cells: a seeded random
    search (after p - 1, h and 0 everywhere) scored by the largest peak / bound ratio of partial_model"""
    rng = np.random.default_rng(seed)
    rp = rounds_partial(w)
    best, best_rc = -1.0, None
    cands = [[P - 1] * rp, [H] * rp, [0] * rp] + [[int(x) for x in rng.integers(0, P, rp)] for _ in range(tries)]
    for rc in cands:
        rcm = [x * R1 % P for x in rc]
        worst = 0.0
        for e in entries:
            _, peak = partial_model(e, stream, k, rcm, w)
            worst = max(worst, max(1 / m for n, m in margins(peak).items() if n != "entry"))
        if worst > best:
            best, best_rc = worst, rc
    return best_rc, best


# found by search_diag(w, seed=w) and search_rc_int(w, ..., seed=w, tries=400) on the entries of entry_patterns for the
# input and external constants of base_tables(w) (test_p2_edges.py::test_the_committed_worst_tables_are_still_the_best)
WORST = {
    24: dict(diag=[471859200] + [74405254] * 23, rc_int=[0] * 21),
    16: dict(diag=[471859200] + [783391594] * 15,
             rc_int=[752221888, 753538400, 824080296, 1239559523, 313946403, 1478014035, 416561508, 1097022247,
                     472592474, 1011147937, 1351591303, 681442665, 1987309909]),
}


def base_tables(w):
    """seeded external constants and input state the aimed cases start from"""
    rng = np.random.default_rng(w)
    ext = [int(x) for x in rng.integers(0, P, 8 * w)]
    inp = [int(x) for x in rng.integers(0, P, w)]
    return ext, inp


def preset_tables(w, m4):
    """the tables the library uses for this instance when none are given (risc0's / SP1's preset), canonical"""
    import p2_chip_ref
    o.oracle_set_params(0 if w == 24 else 1, p2_width=w, p2_m4=m4)
    try:
        rc_ext, rc_int, diag, _ = p2_chip_ref.tables_of()
    finally:
        o.oracle_set_params()
    return [int(x) for x in rc_ext.reshape(-1)], [int(x) for x in rc_int], [int(x) for x in diag]


def table_families(w, m4):
    """name -> (ext, rc_int, diag): the preset, the worst set, random tables"""
    ext, _ = base_tables(w)
    rng = np.random.default_rng(100 + w + m4)
    rp = rounds_partial(w)
    return {"preset": preset_tables(w, m4),
            "worst": (ext, WORST[w]["rc_int"], WORST[w]["diag"]),
            "random": (ext, [int(x) for x in rng.integers(0, P, rp)], [int(x) for x in rng.integers(0, P, w)])}


def aimed_cases(emu, w, m4, families=None, inp=None):
    """[(label, tables, input, raw entry target)]: every table family x every entry pattern, round 3 of the external
    constants solved so that the input enters the partial rounds at the pattern"""
    out = []
    inp = base_tables(w)[1] if inp is None else inp
    for fam, (ext, internal, diag) in (families or table_families(w, m4)).items():
        stream, _ = emul_derived(emu, w, m4, (ext, internal, diag))
        for name, raw in entry_patterns(w, stream).items():
            out.append(("%s/%s" % (fam, name), (aim(inp, m4, ext, target_of_raw(raw)), internal, diag), inp, raw))
    return out


def run_host_cases(emu, ref_emu=None):
    """every aimed case of every instance through `emu`'s permutation against `permute`; the derived words come from
    `ref_emu` (the default build).  -> list of failing labels"""
    bad = []
    for w, m4 in INSTANCES:
        for label, tabs, inp, _ in aimed_cases(ref_emu or emu, w, m4):
            if emul_permute(emu, w, m4, tabs, inp) != permute(inp, m4, *tabs):
                bad.append("%d/%d/%s" % (w, m4, label))
    return bad
