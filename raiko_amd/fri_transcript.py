"""The Fiat-Shamir transcript of the FRI query check as lookup tables: the statement of raiko_amd.fri_open made larger by
the challenger of rk_p3_verify.  In fri_open the query indices sit in free cells of the fold table and every challenge is
a public value that only the host ties to the proof; here the challenger's chain of duplex permutations is a table, the
query indices and the proof-of-work check are cut from its outputs, and beta, zeta, both alpha, the roots, the final
polynomial and the proof-of-work witness are the words that chain absorbs and gives.  Eight tables of one proof:

  fold''      fri_chip.fri_fold_air(..., index_bus=True): fold' plus the column FIRST = REAL SEL[0], with which a query's
              first row receives (Q, IDX) from BUS_FRI_INDEX.
  path, reduce'', ipath   as in fri_open, unchanged.
  transcript  transcript_air: one row per duplex permutation of the DuplexChallenger (csrc/p3_host.hpp), N rows.  IN 16 | OUT 16 |
              STEP one-hot N | REAL | BM 8 | SLOT 8.  STEP is pinned to step 0 on the first row, shifts by one per row and
              is all zero behind N rows; REAL = sum STEP.  The PLAN -- a function of the challenger's calls alone, no
              hashing (plan_of) -- says per step how many words the duplex absorbs and which output cells the samples
              pop.  Per step the constraints select: IN[i] = an observed word (public) for i < n_in; the row before's
              OUT[i] for every other cell; zero for those cells on row 0; OUT[j] = a sampled public value where a
              sample of a field element pops cell j.  BM[j] = [a sample_bits pops cell j at this step], SLOT[j] = its
              slot: constants of the step.  Sends (IN | OUT) on BUS_POSEIDON2_STATE with multiplicity REAL and, per output
              cell j, (SLOT[j], OUT[j]) on BUS_FRI_SAMPLE with multiplicity BM[j].
              Public values: observed | the sampled field elements (pa, pb where a table has lookups, alpha, zeta,
              alpha2, beta of every round).  What sample_bits pops is not public.
  bits        bits_air: one row per sample_bits, queries + 1 rows; slot 0 is the proof of work, slot q + 1 query q.
              SLOT | VALUE | B 31 | H | REAL | QN | IDX | IS_POW | IS_Q.  VALUE = sum 2^i B[i] in the canonical form:
              p - 1 = 0x78000000, so B[30] B[29] B[28] B[27] = 1 forces B[26..0] = 0 (H = B[30] B[29] B[28] keeps it at
              degree 3).  IDX = the low log_max bits on query rows, the low pow_bits bits on the proof-of-work row, where
              it must be 0.  SLOT is 0 on the first row and goes up by one per real row; IS_POW is the first row.
              Receives (SLOT, VALUE) from BUS_FRI_SAMPLE with multiplicity REAL, sends (QN = SLOT - 1, IDX) on
              BUS_FRI_INDEX with multiplicity IS_Q.
  chip        as in fri_open.
  state       p3.poseidon2_chip_air(n_out=16): the sponge's permutations, then the transcript's N.

Still bound on the host (verify_transcript_statement): that the statement's public values are the shard proof's words --
`observed` starts with init, (under a verifying key: the preprocessed root,) the trace root and the tables' public values,
and holds the roots, the final polynomial and the witness where the verifier reads them --, and A and S of the reduce
table, which follow from alpha2, zeta and the opened values at zeta.  Outside: the constraint identity at zeta (reason 3).  The opened values are not observed; this restates
the protocol, it does not change it.

Under a verifying key (statement(..., prep_root=key.root)): the opened preprocessed rows are absorbed and walked up to a
root that is a public value (fri_open); that root is the first thing the challenger's chain observes behind init, so
every challenge depends on it; and the host binds it to the key the caller trusts -- verify_transcript_statement checks
the observed segment against the caller's prep_root and against the root ipath takes.  Still outside: A and S, equality of
the public values with the proof's words, and the constraint identity.

Scope: fri_open's and pow_bits <= 27 (0 included: the witness is still observed and a sample is still popped).

statement / airs / witness / host_tables / device_tables / prove / verify_transcript_statement / sizes / heights are the
calls."""
import collections
import ctypes as C

import numpy as np

from . import _lib, p3
from . import fri_chip as F
from . import fri_open as H
from . import fri_reduce as G
from . import fri_tables as T
from .fri_chip import BUS_FRI_INDEX, BUS_FRI_SAMPLE
from .fri_reduce import BUS_POSEIDON2_STATE
from .p3 import P, AirBuilder

OBSERVE, SAMPLE, SAMPLE_BITS = 0, 1, 2
# a duplex permutation: it absorbs observed[obs_off: obs_off + n_in]; pub = {output cell: index among the sampled field
# elements}, bits = {output cell: slot of the sample_bits that pops it}
Step = collections.namedtuple("Step", "n_in obs_off pub bits")
Plan = collections.namedtuple("Plan", "steps n_obs n_pub n_bits pow_bits")


def plan_of(ops, log_max=None):
    """the duplex permutations from the challenger's calls [(kind, count)]: DuplexChallenger replayed without hashing.  The
    sample_bits come last: the proof of work, then one per query."""
    steps, n_in, n_out, n_obs, n_pub, n_bits, pow_bits = [], 0, 0, 0, 0, 0, 0

    def duplex():
        nonlocal n_in, n_out
        steps.append(Step(n_in, n_obs - n_in, {}, {}))
        n_in, n_out = 0, 8

    for kind, count in ops:
        if kind == OBSERVE:
            assert count > 0 and not n_bits
            for _ in range(count):
                n_out, n_in, n_obs = 0, n_in + 1, n_obs + 1
                if n_in == 8:
                    duplex()
            continue
        assert kind == SAMPLE_BITS or (kind == SAMPLE and count > 0 and not n_bits)
        for _ in range(count if kind == SAMPLE else 1):
            if n_in or not n_out:
                duplex()
            n_out -= 1
            if kind == SAMPLE:
                steps[-1].pub[n_out] = n_pub
                n_pub += 1
            else:
                if n_bits == 0:
                    pow_bits = count
                assert count <= 27 and (n_bits == 0 or log_max is None or count == log_max)
                steps[-1].bits[n_out] = n_bits
                n_bits += 1
    return Plan(steps, n_obs, n_pub, n_bits, pow_bits)


class TranscriptCols:
    IN, OUT, STEP = 0, 16, 32

    def __init__(self, n_steps):
        self.REAL = 32 + n_steps
        self.BM, self.SLOT = self.REAL + 1, self.REAL + 9
        self.width = self.REAL + 17


class BitsCols:
    SLOT, VALUE, B, H, REAL, QN, IDX, IS_POW, IS_Q = 0, 1, 2, 33, 34, 35, 36, 37, 38
    width = 39


def transcript_air(plan, ext_w=p3.EXT_W):
    """the challenger's chain (module docstring).  Every constraint has degree <= 3."""
    steps = plan.steps
    N = len(steps)
    c = TranscriptCols(N)
    b = AirBuilder(c.width, plan.n_obs + plan.n_pub, ext_w)
    loc, nxt = b.local, b.next
    step, nstep = [loc(c.STEP + s) for s in range(N)], [nxt(c.STEP + s) for s in range(N)]
    real = loc(c.REAL)
    for v in step + [real]:
        b.assert_zero(v * (v - 1))
    b.assert_eq(real, F._sum(step))
    b.when_first_row().assert_eq(step[0], b.const(1))
    tr = b.when_transition()
    tr.assert_zero(nstep[0])
    for s in range(N - 1):
        tr.assert_eq(nstep[s + 1], step[s])
    zero = b.const(0)
    for i in range(16):
        absorbs = [s for s in range(N) if i < steps[s].n_in]
        if absorbs:
            b.assert_zero(F._sum([step[s] * (loc(c.IN + i) - b.public(steps[s].obs_off + i)) for s in absorbs]))
        if 0 not in absorbs:
            b.assert_zero(step[0] * loc(c.IN + i))
        keeps = [s for s in range(1, N) if s not in absorbs]
        if keeps:
            tr.assert_zero(F._sum([nstep[s] for s in keeps]) * (nxt(c.IN + i) - loc(c.OUT + i)))
    for j in range(8):
        pops = [s for s in range(N) if j in steps[s].pub]
        if pops:
            b.assert_zero(F._sum([step[s] * (loc(c.OUT + j) - b.public(plan.n_obs + steps[s].pub[j])) for s in pops]))
        cuts = [s for s in range(N) if j in steps[s].bits]
        b.assert_eq(loc(c.BM + j), F._sum([step[s] for s in cuts] or [zero]))
        b.assert_eq(loc(c.SLOT + j), F._sum([step[s] * steps[s].bits[j] for s in cuts if steps[s].bits[j]] or [zero]))
    b.send(BUS_POSEIDON2_STATE, list(range(32)), mult=c.REAL, mult_is_const=False)
    for j in range(8):
        b.send(BUS_FRI_SAMPLE, [c.SLOT + j, c.OUT + j], mult=c.BM + j, mult_is_const=False)
    return b.build()


def bits_air(log_max, pow_bits, ext_w=p3.EXT_W):
    """one row per sample_bits (module docstring).  Every constraint has degree <= 3."""
    c = BitsCols
    b = AirBuilder(c.width, 0, ext_w)
    loc, nxt = b.local, b.next
    bits = [loc(c.B + i) for i in range(31)]
    real, is_pow, is_q, slot, idx, h = loc(c.REAL), loc(c.IS_POW), loc(c.IS_Q), loc(c.SLOT), loc(c.IDX), loc(c.H)
    for v in bits + [real, is_pow, is_q]:
        b.assert_zero(v * (v - 1))
    b.assert_eq(real, is_pow + is_q)
    b.assert_eq(loc(c.VALUE), F._sum([bits[i] * (1 << i) for i in range(31)]))
    # the canonical form: a value >= p = 0x78000001 has B[30..27] set and one of the lower bits
    b.assert_eq(h, bits[30] * bits[29] * bits[28])
    b.assert_zero(h * bits[27] * F._sum(bits[:27]))
    low = lambda n: F._sum([bits[i] * (1 << i) for i in range(n)] or [b.const(0)])
    b.assert_zero(is_q * (idx - low(log_max)))
    b.assert_zero(is_pow * (idx - low(pow_bits)))
    b.assert_zero(is_pow * idx)
    b.assert_zero(is_q * (loc(c.QN) - slot + 1))
    b.when_first_row().assert_eq(is_pow, b.const(1))
    b.when_first_row().assert_zero(slot)
    tr = b.when_transition()
    tr.assert_zero(nxt(c.IS_POW))
    tr.assert_zero(nxt(c.REAL) * (1 - real))
    tr.assert_zero(nxt(c.REAL) * (nxt(c.SLOT) - slot - 1))
    b.receive(BUS_FRI_SAMPLE, [c.SLOT, c.VALUE], mult=c.REAL, mult_is_const=False)
    b.send(BUS_FRI_INDEX, [c.QN, c.IDX], mult=c.IS_Q, mult_is_const=False)
    return b.build()


# ---------------------------------------------------------------------------------------------- the statement
def fri_transcript(tables, proof, init=(), params=None, prep_root=None):
    """rk_p3_fri_transcript (with prep_root, the verifying key's root: rk_p3_fri_transcript_key) -> (verdict, Shape or None,
    ops, observed, sampled): Montgomery words; nothing but the verdict unless it is 0"""
    return T.capture("rk_p3_fri_transcript", 3, tables, proof, init, params, prep_root)


def _check_scope(params):
    H._check_scope(params)
    if params is not None and params.pow_bits > 27:
        raise _lib.RkError(_lib.RK_ERR_INVALID, "the bits table needs pow_bits <= 27")


class Statement:
    """what the eight tables state about one shard proof: fri_open's statement (`opn`) and, from rk_p3_fri_transcript, the
    challenger's calls, the words it observed and the field elements it sampled (Montgomery words)"""

    def __init__(self, opn, ops, observed, sampled):
        self.opn, self.red, self.fold, self.shape, self.params = opn, opn.red, opn.fold, opn.shape, opn.params
        self.ext_w = opn.ext_w
        self.ops_words = np.ascontiguousarray(ops, dtype=np.uint32)
        self.observed = np.ascontiguousarray(observed, dtype=np.uint32)
        self.sampled = np.ascontiguousarray(sampled, dtype=np.uint32)
        self.ops = [tuple(int(v) for v in o) for o in p3.from_mont(self.ops_words).reshape(-1, 2)]
        self.plan = plan_of(self.ops, self.shape.log_max)
        assert self.plan.n_obs == self.observed.size and self.plan.n_pub + self.plan.n_bits == self.sampled.size
        assert self.plan.n_bits == self.shape.queries + 1

    init = property(lambda self: self.opn.init)

    @property
    def transcript_publics(self):
        """observed | the sampled field elements"""
        return np.concatenate([self.observed, self.sampled[: self.plan.n_pub]])


def statement(tables, proof, init=(), params=None, prep_root=None):
    """the statement about the shard proof `proof` of `tables` (raises unless rk_p3_verify accepts it; prep_root: the
    verifying key's root of a proof with preprocessed columns, rk_p3_verify_key)"""
    _check_scope(params)
    opn = H.statement(tables, proof, init, params, prep_root)
    rc, shape, ops, obs, smp = fri_transcript(tables, proof, init, params, prep_root)
    if rc != 0 or shape != opn.shape:
        raise _lib.RkError(_lib.RK_ERR_VERIFY, "the shard proof is refused with reason %d" % rc)
    return Statement(opn, ops, obs, smp)


def heights(st):
    """log heights of (fold'', path, reduce'', ipath, transcript, bits, chip, state)"""
    h_fold, h_path, h_reduce, h_ipath, h_chip, _ = H.heights(st.opn)
    n_state = st.shape.queries * st.opn.perms_per_query + len(st.plan.steps)
    return (h_fold, h_path, h_reduce, h_ipath, F._log_height(len(st.plan.steps)), F._log_height(st.shape.queries + 1), h_chip,
            F._log_height(n_state))


_AIRS = {}


def airs(st):
    """the eight AIRs of a statement (kept per shape, schedule, calls and parameter set)"""
    o, par = st.opn, st.params
    addr = lambda ptr: C.cast(ptr, C.c_void_p).value
    key = (st.shape, tuple(o.slots), tuple(o.batches), st.ext_w, o.coset_shift, tuple(st.ops),
           None if par is None else (par.p2_m4, addr(par.p2_rc_ext), addr(par.p2_rc_int), addr(par.p2_diag)))
    if key not in _AIRS:
        _, path, reduce, ipath, chip, state = H.airs(o)
        _AIRS[key] = (F.fri_fold_air(st.shape, st.ext_w, coset_shift=o.coset_shift, index_bus=True), path, reduce, ipath,
                      transcript_air(st.plan, st.ext_w), bits_air(st.shape.log_max, st.plan.pow_bits, st.ext_w), chip, state)
    return _AIRS[key]


def public_values(st):
    """Montgomery public values per table"""
    none = np.zeros(0, dtype=np.uint32)
    return [st.fold.publics, st.fold.roots, st.red.reduce_publics, st.opn.ipath_publics, st.transcript_publics, none, none, none]


# ---------------------------------------------------------------------------------------------- the numpy witness
def chain_rows(st, consts):
    """the plan replayed with the module's own Poseidon2 restatement -> (transcript rows, bits rows, the 16 cells entering
    every permutation): canonical, padded.  Reproduces `sampled`."""
    plan, sh = st.plan, st.shape
    N = len(plan.steps)
    c, bc = TranscriptCols(N), BitsCols
    h = heights(st)
    rows = np.zeros((1 << h[4], c.width), dtype=np.uint64)
    bits = np.zeros((1 << h[5], bc.width), dtype=np.uint64)
    sin = np.zeros((N, 16), dtype=np.uint64)
    obs = p3.from_mont(st.observed).astype(np.uint64)
    smp = [int(v) for v in p3.from_mont(st.sampled)]
    state = np.zeros(16, dtype=np.uint64)
    value = {}
    for s, stp in enumerate(plan.steps):
        state[: stp.n_in] = obs[stp.obs_off: stp.obs_off + stp.n_in]
        rows[s, c.IN: c.IN + 16] = sin[s] = state
        state = H._permute16(state[None, :], consts)[0].copy()
        rows[s, c.OUT: c.OUT + 16] = state
        rows[s, c.STEP + s], rows[s, c.REAL] = 1, 1
        for cell, k in stp.pub.items():
            assert int(state[cell]) == smp[k], "the replayed chain does not reproduce a sampled field element"
        for cell, slot in stp.bits.items():
            rows[s, c.BM + cell], rows[s, c.SLOT + cell] = 1, slot
            value[slot] = int(state[cell])
            assert value[slot] == smp[plan.n_pub + slot], "the replayed chain does not reproduce a sample_bits"
    for slot in range(sh.queries + 1):
        bits[slot] = bits_row(slot, value[slot], sh.log_max, plan.pow_bits)
    return rows, bits, sin


def bits_row(slot, value, log_max, pow_bits):
    """the bits row of `slot` for a cell holding `value` (canonical)"""
    bc = BitsCols
    row = np.zeros(bc.width, dtype=np.uint64)
    row[bc.SLOT], row[bc.VALUE], row[bc.REAL] = slot, value, 1
    for i in range(31):
        row[bc.B + i] = (value >> i) & 1
    row[bc.H] = int((value >> 28) & 7 == 7)
    row[bc.QN] = slot - 1 if slot else 0
    row[bc.IDX] = value & ((1 << (log_max if slot else pow_bits)) - 1)
    row[bc.IS_POW], row[bc.IS_Q] = int(slot == 0), int(slot != 0)
    return row


def witness(st, chain=None):
    """canonical rows of [fold'', path, reduce'', ipath, transcript, bits, chip, state], padded to their heights (uint64
    arrays).  chain: a statement of the same shape whose transcript, bits and transcript permutations to use in place of
    this one's -- what a test needs to put an honest chain beside the query rows of another proof."""
    consts = F.poseidon2_tables(st.params)
    sh, o = st.shape, st.opn
    fold, path, reduce, ipath, chip, state = H.witness(o)
    fc = F.FoldCols(sh)
    fold = np.concatenate([fold, fold[:, fc.SEL: fc.SEL + 1]], axis=1)             # FIRST = REAL SEL[0]
    trn, bits, tin = chain_rows(st if chain is None else chain, consts)
    if chain is None:
        idx = p3.from_mont(st.fold.records.reshape(sh.queries, -1)[:, 0])
        assert np.array_equal(bits[1: sh.queries + 1, BitsCols.IDX], idx.astype(np.uint64)), "the indices cut from the chain are not the fold table's"
        assert bits[0, BitsCols.IDX] == 0
    n_sponge = sh.queries * o.perms_per_query
    n_state = 1 << heights(st)[7]
    pad = F.chip_rows(np.zeros((1, 16), dtype=np.uint64), consts, [0])
    state = np.concatenate([state[:n_sponge], F.chip_rows(tin, consts), np.repeat(pad, n_state - n_sponge - tin.shape[0], axis=0)])
    return [fold, path, reduce, ipath, trn, bits, chip, state]


TABLE_NAMES = ("fold", "path", "reduce", "ipath", "transcript", "bits", "chip", "state")


def _lead(st):
    return G._lead(st.opn) + (st.ops_words.ctypes.data_as(_lib.u32p), len(st.ops))


def device_inputs(st):
    """the seven host arrays rk_fri_transcript_rows_device reads, in argument order"""
    return H.device_inputs(st.opn) + (st.observed,)


def tables_from_rows(st, rows, publics=None):
    """p3 tables over canonical rows (the witness or a variation of it)"""
    return T.tables_from_rows(airs(st), rows, public_values(st) if publics is None else publics)


def host_tables(st):
    """the eight tables with the numpy witness as host traces"""
    return tables_from_rows(st, witness(st))


def _pinned_tables(st):
    return T.pinned_tables(airs(st), public_values(st), heights(st))


# ---------------------------------------------------------------------------------------------- GPU rows and proof
def sizes(st):
    """rk_fri_transcript_sizes -> dict (the roots must be in the form the plan reports: fri_open.sizes)"""
    sz = T.sizes(_lib.RkFriTranscriptSizeInfo, "rk_fri_transcript_sizes", _lead(st))
    assert sz["roots_words"] == st.opn.in_roots.size and sz["log_kmax"] == st.opn.log_kmax
    return sz


def device_tables(hal, st):
    """rk_fri_transcript_rows_device under hal's parameter set -> [(DeviceBuffer, log_height)] for the eight tables: the
    rows stay in HBM, ready as on_device tables"""
    return T.device_tables(hal, TABLE_NAMES, sizes(st), "rk_fri_transcript_rows_device", _lead(st), device_inputs(st))


def prove(hal, st, device=None):
    """the statement's proof by rk_p3_prove over the eight on_device tables (device: device_tables' result, kept by the
    caller, or None to write the rows now)"""
    return T.prove(hal, _pinned_tables(st), st.init, device if device is not None else device_tables(hal, st))


def observed_segments(st, n_init, n_public):
    """where the verifier's observes lie in `observed`, from the shape, the layout and the tables' public-value counts
    (n_public, per table) -> dict name: (offset, words); None unless the calls are the sequence of rk_p3_verify.  Where a
    table has preprocessed columns the verifying key's root is observed between init and the trace root."""
    sh = st.shape
    R = sh.n_rounds
    n_perm = sum(m.batch == 1 for m in st.opn.layout)
    prep = (("prep_root", 8),) if any(m.batch == 3 for m in st.opn.layout) else ()
    ops = [(OBSERVE, n_init)] + [(OBSERVE, 8)] * len(prep) + [(OBSERVE, 8)] + [(OBSERVE, n) for n in n_public]
    if n_perm:
        ops += [(SAMPLE, 4), (SAMPLE, 4), (OBSERVE, 8)] + [(OBSERVE, 4)] * n_perm
    ops += [(SAMPLE, 4), (OBSERVE, 8), (SAMPLE, 4), (SAMPLE, 4)] + [(OBSERVE, 8), (SAMPLE, 4)] * R + [(OBSERVE, 4), (OBSERVE, 1)]
    ops += [(SAMPLE_BITS, st.plan.pow_bits)] + [(SAMPLE_BITS, sh.log_max)] * sh.queries
    if st.ops != [o for o in ops if o[0] != OBSERVE or o[1]]:
        return None
    seg, at = {}, 0
    for name, n in (("init", n_init),) + prep + (("trace_root", 8), ("public_values", sum(n_public))) + \
                   ((("perm_root", 8), ("cumsums", 4 * n_perm)) if n_perm else ()) + \
                   (("quotient_root", 8), ("commit_roots", 8 * R), ("final_poly", 4), ("witness", 1)):
        seg[name] = (at, n)
        at += n
    assert at == st.observed.size
    return seg


def verify_transcript_statement(tables, shard_proof, init, fri_proof, params=None, prep_root=None) -> int:
    """0 iff fri_proof proves, for shard_proof, what verify_open_statement states and that the query indices, the proof of
    work, beta, zeta, both alpha, the roots and the final polynomial are what rk_p3_verify's challenger gives over the words
    it observes.  Everything is recomputed from the shard proof through the four capture calls; the segments of `observed`
    and `sampled` are checked word for word against the public values the other tables take (the same Montgomery arrays
    go to both sides: that is the in-STARK link), `observed` must start with init, the trace root and the tables' public
    values, all eight heights are pinned, and fri_proof is verified against them.  Otherwise the reason (rk_p3_verify's
    numbering, as verify_open_statement; 1 where the captures do not fit each other).  prep_root: the verifying key's root
    of a shard proof with preprocessed columns, the root the caller trusts: the observed segment behind init must be
    that root, and so must the public value the preprocessed tree of ipath ends in."""
    _check_scope(params)
    rc, shape, pub, rec = F.fri_openings(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    rc, shape2, layout, in_pub, in_rec = G.fri_inputs(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    rc, shape3, roots, paths = H.fri_input_paths(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    rc, shape4, ops, obs, smp = fri_transcript(tables, shard_proof, init, params, prep_root)
    if rc != 0:
        return rc
    return _check_bound(tables, init, fri_proof, params, prep_root, (shape, pub, rec), (shape2, layout, in_pub, in_rec), (shape3, roots, paths),
                        (shape4, ops, obs, smp))


def _check_bound(tables, init, fri_proof, params, prep_root, openings, inputs, in_paths, transcript) -> int:
    """verify_transcript_statement behind its four captures (shape and arrays of each): the host-side binding, then the
    proof.  On its own so that a test can hand it captures that were tampered with."""
    (shape, pub, rec), (shape2, layout, in_pub, in_rec), (shape3, roots, paths), (shape4, ops, obs, smp) = openings, inputs, in_paths, transcript
    if shape2 != shape or shape3 != shape or shape4 != shape or not G._check_zeta(in_pub):
        return 1
    if not H._roots_bound(roots, prep_root):
        return 1
    opn = H.Statement(G.Statement(F.Statement(shape, pub, rec, params), layout, in_pub, in_rec, params), roots, paths)
    st = Statement(opn, ops, obs, smp)
    iw = np.ascontiguousarray(init, dtype=np.uint32).reshape(-1)
    pvs = np.concatenate([np.zeros(0, dtype=np.uint32)] + [np.ascontiguousarray(t.public_values, dtype=np.uint32).reshape(-1) for t in tables])
    seg = observed_segments(st, iw.size, [int(np.asarray(t.public_values).size) for t in tables])
    if seg is None:
        return 1
    R = shape.n_rounds
    n_perm = sum(m.batch == 1 for m in layout)
    at = lambda name: st.observed[seg[name][0]: seg[name][0] + seg[name][1]]
    s0 = 8 if n_perm else 0                                  # pa, pb come first where a table has lookups
    if st.plan.n_pub != s0 + 12 + 4 * R:
        return 1
    ok = np.array_equal(at("init"), iw) and np.array_equal(at("trace_root"), roots[:8]) and np.array_equal(at("public_values"), pvs)
    if prep_root is not None:                                # the key the caller trusts, where the chain observes it and where ipath ends
        kr = np.ascontiguousarray(prep_root, dtype=np.uint32).reshape(-1)
        ok = ok and "prep_root" in seg and np.array_equal(at("prep_root"), kr) and np.array_equal(at("prep_root"), roots[25:33])
    else:
        ok = ok and "prep_root" not in seg
    ok = ok and np.array_equal(at("quotient_root"), roots[16:24]) and (not n_perm or np.array_equal(at("perm_root"), roots[8:16]))
    ok = ok and np.array_equal(at("commit_roots"), st.fold.roots) and np.array_equal(at("final_poly"), st.fold.publics[12 * R:])
    zeta, alpha2 = st.sampled[s0 + 4: s0 + 8], st.sampled[s0 + 8: s0 + 12]
    ok = ok and np.array_equal(np.concatenate([alpha2, zeta]), st.red.reduce_publics[:8])
    ok = ok and np.array_equal(st.sampled[s0 + 12: s0 + 12 + 4 * R], st.fold.publics[: 4 * R])
    if not ok:
        return 1
    return p3.verify(_pinned_tables(st), fri_proof, st.init, params=params)
