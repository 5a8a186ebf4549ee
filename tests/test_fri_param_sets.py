"""The census of the FRI row kernels that exist in two instantiations, as code (the style of tests/test_launch_thresholds.py):
four kernels of csrc/fri_tables.hip are chosen at run time by the external matrix of the context's Poseidon2 (p2_m4).  This
file reads the sites that choose out of the source and proves, without a GPU, that fri_param_sets.KERNEL_ARMS names GPU
test ids for both arms of each, that those ids exist, and that every parameter set reaches the rows test of every statement.

  fri_tables.hip   launch_m4(... k<0>, k<1> ...)           fri_path_kernel, fri_open_sponge_kernel, fri_open_ipath_kernel
  fri_tables.hip   fri_transcript_chain_kernel<p2::K2|K3>  the two arms of FriCall::transcript"""
import importlib
import os
import re

import numpy as np
import pytest

import fri_param_sets as PS
import oracle_lib as o
from raiko_amd import hal, p3

SOURCE = os.path.join(o.ROOT, "raiko_amd", "csrc", "fri_tables.hip")
STATEMENTS = ("chip", "reduce", "open", "transcript")


def call_sites(src):
    """-> ({kernel: (name of the <0> arm, name of the <1> arm)} of every launch_m4( call, chain instantiations launched):
    every `launch_m4(` but the template's own definition must parse, so that a new site cannot pass unseen"""
    sites = {}
    for m in re.finditer(r"launch_m4\(", src):
        line_start = src.rfind("\n", 0, m.start()) + 1
        if src[line_start: m.start()].strip() == "int":                  # the definition: `int launch_m4(rk_ctx* ctx, ...`
            continue
        call = re.match(r'launch_m4\(ctx, "(\w+)", (\w+)<0>, (\w+)<1>,', src[m.start():])
        assert call, "a launch_m4( site this census cannot read: " + src[m.start(): m.start() + 120]
        name, k0, k1 = call.groups()
        assert name not in sites, name
        sites[name] = (k0, k1)
    chain = re.findall(r'launch\(ctx, "fri_transcript_chain_kernel", fri_transcript_chain_kernel<p2::(\w+)>', src)
    return sites, chain


def rows_ids(statement):
    """the ids of the rows test under parameter sets of one statement's GPU file, read from its parametrize list"""
    mod = importlib.import_module("test_gpu_fri_" + statement)
    marks = [m for m in mod.test_gpu_rows_under_parameter_sets.pytestmark if m.name == "parametrize"]
    assert len(marks) == 1 and marks[0].args[0] == "pset,case"
    pairs, ids = list(marks[0].args[1]), list(marks[0].kwargs["ids"])
    assert len(pairs) == len(ids) == len(set(ids))
    return {"tests/test_gpu_fri_%s.py::test_gpu_rows_under_parameter_sets[%s]" % (statement, i): pair for i, pair in zip(ids, pairs)}


def test_every_two_instantiation_kernel_has_ids_for_both_arms():
    sites, chain = call_sites(open(SOURCE).read())
    assert len(sites) == 3 and all(k0 == k1 == name for name, (k0, k1) in sites.items())   # <0> first: k0 is the m4 = 0 arm
    assert sorted(chain) == sorted(PS.CHAIN_ARMS.values()) == ["K2", "K3"]
    assert set(PS.KERNEL_ARMS) == set(sites) | {"fri_transcript_chain_kernel"}
    known = {}
    for s in STATEMENTS:
        known.update(rows_ids(s))
    for kernel, arms in PS.KERNEL_ARMS.items():
        assert set(arms) == {0, 1}
        for m4, ids in arms.items():
            assert ids, (kernel, m4)
            for i in ids:
                assert i in known, i
                pset, case = known[i]
                assert PS.shard_params(pset, case)[1].get("p2_m4", 1) == m4, (kernel, i)     # preset 1's own matrix is 1
    # the statements whose stages launch each kernel (FriCall::commit / open / transcript)
    stage = {"fri_path_kernel": STATEMENTS, "fri_open_sponge_kernel": ("open", "transcript"), "fri_open_ipath_kernel": ("open", "transcript"),
             "fri_transcript_chain_kernel": ("transcript",)}
    for kernel, arms in PS.KERNEL_ARMS.items():
        for ids in arms.values():
            assert {i.split("::")[0] for i in ids} == {"tests/test_gpu_fri_%s.py" % s for s in stage[kernel]}


def test_a_new_site_without_a_row_fails_the_census():
    src = open(SOURCE).read()
    more = src + '\nint f(rk_ctx* ctx) { return launch_m4(ctx, "fri_new_kernel", fri_new_kernel<0>, fri_new_kernel<1>, dim3(1), dim3(64)); }\n'
    sites, _ = call_sites(more)
    assert "fri_new_kernel" in sites and "fri_new_kernel" not in PS.KERNEL_ARMS
    with pytest.raises(AssertionError):
        call_sites(src + "\nint g(rk_ctx* ctx) { return launch_m4(ctx, name, a, b, dim3(1), dim3(64)); }\n")


def test_every_set_reaches_the_rows_of_every_statement():
    for s in STATEMENTS:
        used = {pset for pset, _ in rows_ids(s).values()}
        assert used == set(PS.PARAM_SETS), s
        assert sorted(rows_ids(s).values()) == sorted(PS.ROW_IDS)
    for pset, cases in PS.SET_SHARDS.items():
        assert cases and all(c in PS.TRANSCRIPT_SHARDS for c in cases)
    import test_gpu_fri_key as K
    assert PS.KEYED_CASE in K.ROW_CASES and PS.KEYED_SET == PS.SHARED_SET == "m4_0" and set(PS.PROVE_SETS) == {"m4_0", "risc0_field"}


def test_custom_tables_differ_from_the_built_in_ones_in_every_array():
    custom, builtin = PS.custom_tables_canonical(), PS.builtin_tables_canonical()
    for name, n in PS.TABLE_SIZES:
        assert custom[name].shape == builtin[name].shape == (n,) and int(custom[name].max()) < PS.P
        assert not np.any(custom[name] == builtin[name]), name                # not one word in common
    for pset in ("m4_0_tables", "m4_1_tables"):
        preset, over = PS.shard_params(pset, PS.SMALL_SHARDS[0])
        blob = hal.make_params(preset, **over)
        for name, n in PS.TABLE_SIZES:
            words = np.ctypeslib.as_array(getattr(blob, name), shape=(n,))
            assert np.array_equal(p3.from_mont(words), custom[name])         # passed as Montgomery words
    assert PS.PARAM_SETS["m4_0_tables"][1]["p2_m4"] == 0 and PS.PARAM_SETS["m4_1_tables"][1]["p2_m4"] == 1


def test_risc0_field_differs_from_preset_1_in_w_root_and_shift():
    case = PS.SMALL_SHARDS[0]
    a = hal.make_params(1, **PS.preset1_params("risc0_field", case)[1])
    b = hal.make_params(1, **PS.shard_params("risc0_field", case)[1])
    r0 = hal.make_params(0)
    assert (b.ext_w, b.root_2_27, b.coset_shift) == (r0.ext_w, r0.root_2_27, r0.coset_shift) == (PS.P - 11, 137, 3)
    assert a.ext_w != b.ext_w and a.root_2_27 != b.root_2_27 and a.coset_shift != b.coset_shift
    assert (b.p2_width, b.p2_m4, b.p2_pad_free, b.fri_fold_log2, b.blowup_log2) == (16, 1, 1, 1, 1) == (a.p2_width, a.p2_m4, a.p2_pad_free, a.fri_fold_log2, a.blowup_log2)
    for pset in ("blow3", "blow4"):
        assert PS.shard_params(pset, PS.SET_SHARDS[pset][0])[1]["blowup_log2"] == int(pset[-1])
