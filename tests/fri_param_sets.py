"""The parameter sets the FRI statements (raiko_amd/fri_chip.py, fri_reduce.py, fri_open.py, fri_transcript.py) are tested
under beside SP1's preset, shared by the CPU tests (tests/test_fri_*.py), the GPU tests (tests/test_gpu_fri_*.py) and the
census (tests/test_fri_param_sets.py).  Four row kernels of csrc/fri_tables.hip exist in two instantiations chosen at run
time by the external matrix of the context's width-16 Poseidon2 (p2_m4); the scope of the statements (fri_scope) admits
either, any round-constant tables, any field and blow-ups 1 to 4.

  m4_0          the other external matrix: the <0> instantiations, the K2 arm of the chain kernel
  m4_0_tables   ... with round constants and diagonal of its own (p2_chip_tab / p2_chip_layout read the blob's)
  m4_1_tables   SP1's matrix with the same tables
  risc0_field   x^4 + 11, risc0's root of unity and coset shift, under the width-16 hash and the fold by two
  blow3, blow4  SP1's preset at blow-up 8 and 16: two cases of tests/p3_cases.py as they stand"""
import numpy as np

from p3_cases import P3_CASES, init_of, tables_of
from raiko_amd import fri_chip as F
from raiko_amd import p3

P = p3.P
TABLE_SEED = 20260
TABLE_SIZES = (("p2_rc_ext", 128), ("p2_rc_int", 13), ("p2_diag", 16))


def custom_tables_canonical():
    """round constants and diagonal from a seeded generator, every word canonical (< p): name -> uint64 array"""
    rng = np.random.default_rng(TABLE_SEED)
    return {name: rng.integers(1, P, size=n).astype(np.uint64) for name, n in TABLE_SIZES}


def custom_tables():
    """the same as Montgomery words, the form rk_params and the oracle's blob take"""
    return {name: p3.to_mont(a) for name, a in custom_tables_canonical().items()}


def builtin_tables_canonical():
    rc_ext, rc_int, diag, _ = F.poseidon2_tables(None)
    return {"p2_rc_ext": rc_ext.reshape(-1), "p2_rc_int": rc_int, "p2_diag": diag}


RISC0_FIELD = dict(ext_w=P - 11, root_2_27=137, coset_shift=3)          # preset 0's: x^4 + 11

# name -> (preset, overrides on top of the shard case's own)
PARAM_SETS = {
    "m4_0": (1, dict(p2_width=16, p2_m4=0, p2_pad_free=1)),
    "m4_0_tables": (1, dict(p2_width=16, p2_m4=0, p2_pad_free=1, **custom_tables())),
    "m4_1_tables": (1, dict(p2_width=16, p2_m4=1, p2_pad_free=1, **custom_tables())),
    "risc0_field": (1, dict(RISC0_FIELD, p2_width=16, p2_m4=1, p2_pad_free=1, fri_fold_log2=1, blowup_log2=1)),
    "blow3": (P3_CASES["sp1_blow3_deg9_deg5_cubic"][0], dict(P3_CASES["sp1_blow3_deg9_deg5_cubic"][1])),
    "blow4": (P3_CASES["sp1_blow4_lookup_beside_deg9"][0], dict(P3_CASES["sp1_blow4_lookup_beside_deg9"][1])),
}
# the preset whose extension the AIRs with interactions are written for (tests/p3_cases.py EXT_W)
AIR_PRESET = {"risc0_field": 0}
# sets that differ from preset 1 only by overrides their cases already carry: their proofs are preset 1's
PLAIN_PRESET_SETS = ("blow3", "blow4")

# two heights (a reduced opening joins mid-chain, a shorter matrix is injected into the input path); a permutation batch
SMALL_SHARDS = ["sp1_mixed_fib8_cubic4", "sp1_lookup_beside_plain"]
SET_SHARDS = {"m4_0": SMALL_SHARDS, "m4_0_tables": SMALL_SHARDS, "m4_1_tables": SMALL_SHARDS, "risc0_field": SMALL_SHARDS,
              "blow3": ["sp1_blow3_deg9_deg5_cubic"], "blow4": ["sp1_blow4_lookup_beside_deg9"]}
# (set, case) of every rows id, and the ids pytest gives them
ROW_IDS = [(s, c) for s in PARAM_SETS for c in SET_SHARDS[s]]
row_id = lambda pset, case: "%s-%s" % (pset, case)
# the statement proven from device tables under a set: the shard with all three input batches
PROVE_SETS = ["m4_0", "risc0_field"]
PROVE_CASE = "sp1_lookup_beside_plain"
# the transcript statement's shards: (queries, init) of tests/test_gpu_fri_transcript.py ROW_CASES where the case is
# there -- 7 queries: the indices end with the proof-of-work block; 8: one duplex that absorbs nothing --, else the case's own
TRANSCRIPT_SHARDS = {"sp1_mixed_fib8_cubic4": (7, [5, 6, 7]), "sp1_lookup_beside_plain": (8, [1, 2, 3, 4, 5]),
                     "sp1_blow3_deg9_deg5_cubic": (4, []), "sp1_blow4_lookup_beside_deg9": (3, [1])}
# the keyed statement (tests/test_gpu_fri_key.py) and the shared-tables check (tests/test_gpu_fri_transcript.py)
KEYED_SET, KEYED_CASE = "m4_0", "gate_cubic"
SHARED_SET, SHARED_CASE = "m4_0", "sp1_mixed_fib8_cubic4"


def shard_params(pset, case, transcript=False):
    """(preset, overrides) of shard `case` under set `pset`: the case's own queries and proof of work, the set's on top"""
    preset, over = PARAM_SETS[pset]
    assert preset == P3_CASES[case][0] == 1
    out = dict(P3_CASES[case][1], **over)
    if transcript:
        out["queries"] = TRANSCRIPT_SHARDS[case][0]
    assert out["pow_bits"] >= 1                  # the bits table cuts a proof of work
    return preset, out


def preset1_params(pset, case, transcript=False):
    """the same shard's parameters under plain preset 1: what a proof under `pset` must not verify under"""
    out = dict(P3_CASES[case][1])
    if transcript:
        out["queries"] = TRANSCRIPT_SHARDS[case][0]
    return 1, out


def shard_tables(pset, case, transcript=False):
    """(tables, init words) of shard `case` under set `pset`"""
    tables = tables_of(case, AIR_PRESET.get(pset))
    if transcript:
        return tables, p3.to_mont(np.array(TRANSCRIPT_SHARDS[case][1], dtype=np.uint64))
    return tables, init_of(case)


# ---------------------------------------------------------------------------------------------- the census's table
# kernel of csrc/fri_tables.hip with one instantiation per external matrix -> {m4: GPU test ids that launch that arm}.
# fri_path_kernel runs in every statement's commit stage; the sponge and ipath kernels in the open and the transcript
# statement; the chain kernel (K2 for m4 = 0, K3 for m4 = 1) in the transcript statement.
_ROWS = "tests/test_gpu_fri_%s.py::test_gpu_rows_under_parameter_sets[%s]"


def _ids(statements, psets):
    return [_ROWS % (st, row_id(s, c)) for st in statements for s in psets for c in SET_SHARDS[s]]


M4_0_SETS, M4_1_SETS = ["m4_0", "m4_0_tables"], ["m4_1_tables", "risc0_field", "blow3", "blow4"]
KERNEL_ARMS = {
    "fri_path_kernel": {0: _ids(("chip", "reduce", "open", "transcript"), M4_0_SETS), 1: _ids(("chip", "reduce", "open", "transcript"), M4_1_SETS)},
    "fri_open_sponge_kernel": {0: _ids(("open", "transcript"), M4_0_SETS), 1: _ids(("open", "transcript"), M4_1_SETS)},
    "fri_open_ipath_kernel": {0: _ids(("open", "transcript"), M4_0_SETS), 1: _ids(("open", "transcript"), M4_1_SETS)},
    "fri_transcript_chain_kernel": {0: _ids(("transcript",), M4_0_SETS), 1: _ids(("transcript",), M4_1_SETS)},
}
CHAIN_ARMS = {0: "K2", 1: "K3"}        # the instantiation of fri_transcript_chain_kernel per m4


# ---------------------------------------------------------------------------------------------- the CPU check of a set
_PROOFS = {}


def cpu_shard(pset, case, transcript=False):
    """-> (blob, tables, init, the oracle's shard proof): the oracle is left under the set; the proof is made once"""
    import oracle_lib as o
    from raiko_amd import hal
    preset, over = shard_params(pset, case, transcript)
    o.oracle_set_params(preset, **over)
    blob = hal.make_params(preset, **over)
    key = (pset, case, transcript)
    if key not in _PROOFS:
        tables, init = shard_tables(pset, case, transcript)
        _PROOFS[key] = (tables, init, o.oracle_p3_prove(tables, init))
    return (blob,) + _PROOFS[key]


def check_reference(mod, verify_statement, pset, case, transcript=False):
    """the reference alone under a set, for one statement module: the oracle's shard proof is accepted under the set's
    blob and refused under preset 1; the statement is captured; the numpy witness satisfies every AIR; the oracle's proof
    over the witness is accepted by both verifiers (the buses) and by the statement's verifier"""
    import field_ref as FR
    import oracle_lib as o
    from raiko_amd import hal
    blob, tables, init, pf = cpu_shard(pset, case, transcript)
    assert p3.verify(tables, pf, init, params=blob) == 0
    preset, over = preset1_params(pset, case, transcript)
    plain = hal.make_params(preset, **over)
    if pset in PLAIN_PRESET_SETS:
        assert p3.verify(tables, pf, init, params=plain) == 0
    else:
        assert p3.verify(tables, pf, init, params=plain) != 0
    st = mod.statement(tables, pf, init, blob)
    rows = mod.witness(st)
    pvs = [FR.from_mont(v.astype(np.uint64)) for v in mod.public_values(st)]
    for air, r, pv in zip(mod.airs(st), rows, pvs):
        assert air.width == r.shape[1] and air.check_trace(r, pv) == []
    tabs = mod.tables_from_rows(st, rows)
    fp = o.oracle_p3_prove(tabs, st.init)
    assert o.oracle_p3_verify(tabs, fp, st.init) == 0 == p3.verify(tabs, fp, st.init, params=blob)
    assert verify_statement(tables, pf, init, fp, blob) == 0
    return st, rows
