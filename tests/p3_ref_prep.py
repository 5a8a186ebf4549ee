"""TEST INFRASTRUCTURE: tests/p3_ref.py extended by the preprocessed batch (rk_p3_setup / rk_p3_prove_key /
rk_p3_verify_key, include/raiko_hip.h) -- the same exact integer algebra, nothing of the product called, the proof words
only read.  p3_ref.py is imported, not edited.

The protocol as restated here (the header comment and csrc/p3_verify.hip state the same one):

* transcript: the init words; THE PREPROCESSED ROOT if any table has preprocessed columns (it is an input here, as it is
  for the verifier: the proof does not carry it); then the trace root and everything after it as in p3_ref.transcript.
* opened values per table: local 4w | next 4w | [prep local 4c | prep next 4c] | [perm local | perm next] | chunks.
* per query: trace rows, path 8 log_max | [preprocessed rows of every preprocessed table in table order, path
  8 log_kmax, log_kmax = the LDE height of the tallest preprocessed table] | [permutation rows, path 8 log_pmax] |
  quotient rows, path 8 log_max | per round: sibling 4, path 8 (log_max - 1 - round).

The algebra over the preprocessed columns is the algebra over trace columns: PREP_LOCAL / PREP_NEXT a read column a of
the preprocessed matrix the way LOCAL / NEXT read the trace, and an interaction's column c >= width is preprocessed
column c - width.  `joined` therefore restates a table as one over width + prep_width columns (trace | preprocessed,
PREP_* rewritten to LOCAL / NEXT of the shifted column) and hands that to p3_ref's eval_steps, perm_trace,
quotient_chunks and folded_at_zeta; what is NEW -- the transcript, the layout, which values are opened where -- is
written out below.
"""
import numpy as np

import field_ref as F
import p3_ref as R
from raiko_amd import p3

P = F.P


class _View:
    """a table restated for p3_ref: .air, .trace (Montgomery), .public_values, .log_height"""

    def __init__(self, air, trace, public_values, log_height):
        self.air, self.trace, self.public_values, self.log_height = air, trace, public_values, log_height


def joined(table):
    """the table over width + prep_width columns (trace | preprocessed)"""
    air = table.air
    if not air.prep_width:
        return table
    steps = air.steps.copy()
    for op, to in ((p3.PREP_LOCAL, p3.LOCAL), (p3.PREP_NEXT, p3.NEXT)):
        rows = steps[:, 0] == op
        steps[rows, 1] += air.width
        steps[rows, 0] = to
    jair = p3.Air(steps, air.width + air.prep_width, air.n_public, air.interactions)
    return _View(jair, np.concatenate([table.trace, table.prep], axis=1), table.public_values, table.log_height)


# ---------------------------------------------------------------- layout
def proof_words(tables, blowup_log2, queries):
    """the exact size of a proof, counted the way `parse` walks it"""
    nt = len(tables)
    log_h = [t.log_height + blowup_log2 for t in tables]
    log_max = max(log_h)
    perm = [i for i, t in enumerate(tables) if t.air.perm_width]
    prep = [i for i, t in enumerate(tables) if t.air.prep_width]
    head = 1 + nt + 8 + (8 + 4 * len(perm) if perm else 0) + 8
    for t in tables:
        head += 8 * t.air.width + 8 * t.air.prep_width + 8 * t.air.perm_width + (16 << t.air.log_quotient_degree())
    n_rounds = log_max - blowup_log2
    head += 1 + 8 * n_rounds + 4 + 1
    q = sum(t.air.width for t in tables) + 8 * log_max
    if prep:
        q += sum(tables[i].air.prep_width for i in prep) + 8 * max(log_h[i] for i in prep)
    if perm:
        q += sum(tables[i].air.perm_width for i in perm) + 8 * max(log_h[i] for i in perm)
    q += sum(4 << t.air.log_quotient_degree() for t in tables) + 8 * log_max
    q += sum(4 + 8 * (log_max - 1 - r) for r in range(n_rounds))
    return head + queries * q


def parse(tables, words, blowup_log2=None, queries=None):
    """the proof's head as p3_ref.parse gives it, with "prep_local" / "prep_next" per table that has preprocessed
    columns; with blowup_log2 and queries also the word spans of the query part: out["spans"] = {name: (start, end)} for
    "head.t<i>.prep_local", "head.t<i>.prep_next", and per query "q<j>.trace_rows", ".trace_path", ".prep_rows",
    ".prep_path", ".perm_rows", ".perm_path", ".quotient_rows", ".quotient_path", ".fri"; out["end"] = the total"""
    raw = [int(v) for v in words]
    nt = raw[0]
    assert nt == len(tables)
    out = {"log_n": raw[1:1 + nt], "spans": {}}
    w = [int(v) for v in F.from_mont(np.asarray(words, dtype=np.uint64))]
    pos = 1 + nt

    def take(m, name=None):
        nonlocal pos
        pos += m
        if name:
            out["spans"][name] = (pos - m, pos)
        return w[pos - m:pos]

    out["trace_root"] = take(8)
    perm = [t for t in tables if t.air.perm_width]
    if perm:
        out["perm_root"] = take(8)
        out["cumsums"] = [take(4) for _ in perm]
    out["quotient_root"] = take(8)
    ext4 = lambda flat: [tuple(flat[4 * c:4 * c + 4]) for c in range(len(flat) // 4)]
    out["tables"] = []
    for i, t in enumerate(tables):
        wd, cw, pw, qd = t.air.width, t.air.prep_width, t.air.perm_width, 1 << t.air.log_quotient_degree()
        o = {"local": ext4(take(4 * wd)), "next": ext4(take(4 * wd))}
        if cw:
            o["prep_local"] = ext4(take(4 * cw, "head.t%d.prep_local" % i))
            o["prep_next"] = ext4(take(4 * cw, "head.t%d.prep_next" % i))
        if pw:
            o["perm_local"], o["perm_next"] = ext4(take(4 * pw)), ext4(take(4 * pw))
        o["chunks"] = [ext4(take(16)) for _ in range(qd)]
        out["tables"].append(o)
    if blowup_log2 is None:
        return out
    log_h = [k + blowup_log2 for k in out["log_n"]]
    log_max = max(log_h)
    n_rounds = raw[pos]
    assert n_rounds == log_max - blowup_log2
    take(1 + 8 * n_rounds + 4 + 1)
    kh = [log_h[i] for i, t in enumerate(tables) if t.air.prep_width]
    ph = [log_h[i] for i, t in enumerate(tables) if t.air.perm_width]
    for j in range(queries):
        q = "q%d." % j
        take(sum(t.air.width for t in tables), q + "trace_rows")
        take(8 * log_max, q + "trace_path")
        if kh:
            take(sum(t.air.prep_width for t in tables), q + "prep_rows")
            take(8 * max(kh), q + "prep_path")
        if ph:
            take(sum(t.air.perm_width for t in tables), q + "perm_rows")
            take(8 * max(ph), q + "perm_path")
        take(sum(4 << t.air.log_quotient_degree() for t in tables), q + "quotient_rows")
        take(8 * log_max, q + "quotient_path")
        take(sum(4 + 8 * (log_max - 1 - r) for r in range(n_rounds)), q + "fri")
    out["end"] = pos
    return out


# ---------------------------------------------------------------- transcript
def transcript(preset, tables, init_canonical, pf, prep_root_canonical):
    """-> (alpha, zeta, (perm alpha, perm beta) or None): p3_ref.transcript with the preprocessed root observed right
    after the init words"""
    ch = R.Challenger(preset)
    ch.observe(init_canonical)
    if any(t.air.prep_width for t in tables):
        assert prep_root_canonical is not None and len(prep_root_canonical) == 8
        ch.observe(prep_root_canonical)
    else:
        assert prep_root_canonical is None
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


def perm_entries(trace, prep, interactions, chal, W):
    """p3_ref.perm_entries over a canonical main trace (n, width) and preprocessed matrix (n, prep_width): an interaction's
    column c >= width is preprocessed column c - width"""
    return R.perm_entries(np.concatenate([np.asarray(trace, dtype=np.uint64), np.asarray(prep, dtype=np.uint64)], axis=1), interactions, chal, W)


# ---------------------------------------------------------------- the checks
def check_proof(preset, blowup_log2, tables, init_mont, words, prep_root_mont, quotient=True, tall=False, queries=None):
    """p3_ref.check_proof for tables with preprocessed columns (Table.prep): the transcript with the root observed, the
    cumulative sums (interactions may read preprocessed columns), the trace openings, THE PREPROCESSED OPENINGS at zeta and
    zeta * g from the integer interpolation of the preprocessed matrix, the permutation openings, the quotient chunks of
    the AIR with its PREP_* leaves and the recombined identity.  queries: also the total length.  -> (alpha, zeta)"""
    W = R.PRESETS[preset][0]
    pf = parse(tables, words, blowup_log2 if queries is not None else None, queries)
    assert pf["log_n"] == [t.log_height for t in tables]
    if queries is not None:
        assert pf["end"] == len(words) == proof_words(tables, blowup_log2, queries), "proof length"
    root = None if prep_root_mont is None else [int(v) for v in F.from_mont(np.asarray(prep_root_mont, dtype=np.uint64))]
    alpha, zeta, pch = transcript(preset, tables, F.from_mont(np.asarray(init_mont, dtype=np.uint64)), pf, root)
    views = [joined(t) for t in tables]
    ptraces, chal = {}, None
    if pch is not None:
        chal = R.challenge_words(pch, W)
        for pi, ti in enumerate(i for i, t in enumerate(tables) if t.air.perm_width):
            ptraces[ti] = R.perm_trace(views[ti], pch, preset)
            assert pf["cumsums"][pi] == [int(v) for v in ptraces[ti][-1, -4:]], "table %d: cumulative sum" % ti
    for ti, (t, v, op) in enumerate(zip(tables, views, pf["tables"])):
        loc, nxt = R.trace_openings(t, zeta, preset, tall)
        assert op["local"] == loc, "table %d: trace_local" % ti
        assert op["next"] == nxt, "table %d: trace_next" % ti
        kloc, knxt = [], []
        if t.air.prep_width:
            kloc, knxt = R.openings(F.from_mont(t.prep), t.log_height, zeta, preset, tall)
            assert op["prep_local"] == kloc, "table %d: prep_local" % ti
            assert op["prep_next"] == knxt, "table %d: prep_next" % ti
        perm_q = perm_z = None
        if t.air.perm_width:
            ploc, pnxt = R.openings(ptraces[ti], t.log_height, zeta, preset, tall)
            assert op["perm_local"] == ploc, "table %d: perm_local" % ti
            assert op["perm_next"] == pnxt, "table %d: perm_next" % ti
            cs = [int(x) for x in ptraces[ti][-1, -4:]]
            perm_q, perm_z = (ptraces[ti], chal, cs), (ploc, pnxt, chal, cs)
        if not quotient or tall:
            continue
        lqd = t.air.log_quotient_degree()
        want = R.quotient_chunks(v, alpha, zeta, preset, blowup_log2, perm_q)
        for j, (got, exp) in enumerate(zip(op["chunks"], want)):
            assert got == exp, "table %d: quotient chunk %d of %d" % (ti, j, 1 << lqd)
        assert R.recombine(want, zeta, t.log_height, lqd, preset) == R.folded_at_zeta(v, loc + kloc, nxt + knxt, alpha, zeta, preset, perm_z), \
            "table %d: zps recombination" % ti
    return alpha, zeta
