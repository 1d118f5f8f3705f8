"""The check on the checker of the gather / scatter conformance suite; runs without a GPU.
  - numpy emulations of the kernels' arithmetic (util_scatter_ref.emu_*: the tree of the deterministic scatter, the lane / LDS / grid
    split of colsum, the slab order, the slice split of vit_assemble_bwd8, the fp8 decode tables, RNE to bf16) pass the references
    and bounds of the GPU module on the same operands (the printed ratios are the emulation's column of
    profiles/scatter_conformance_worst_ratio.txt);
  - seeded defects, each an emulation with one flaw, are rejected by those checks; `test_defects_the_old_tolerance_accepts` prints
    which of them the assertion of tests/test_ops_gpu.py (max-scaled relerr under its thresholds) would have accepted;
  - the dispatch rules restated in util_scatter_cases.py, each case's claimed instantiation, and the coverage of the build: the set
    in scope is computed from tests/golden/kernel_resources.json by name pattern, so a later instantiation cannot appear without a
    case, and the GPU module's committed kernel listing launches every one of them."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_scatter_cases as SC  # noqa: E402
import util_scatter_ref as SR  # noqa: E402
from util_gemm_ref import check  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERAGE_PROFILE = "profiles/scatter_conformance_kernel_stats.txt"
OLD_TOL = {"f32": 1e-5, "bf16": 1.2e-2}   # tests/test_ops_gpu.py: relerr < 1e-5 on fp32 results, tol(bf16) on bf16 ones


def old_relerr(got, ref):
    """relerr of tests/test_ops_gpu.py"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-6))


def rejected(got, ref, bound, what):
    with pytest.raises(AssertionError):
        check(got, ref, bound, what, log=False)


def cases(table):
    return [(c["name"], dt) for c in table for dt in ([c["only"]] if c.get("only") else SC.DTYPES)]


def bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------------------------------------ emulations within the bounds
@pytest.mark.parametrize("name,dtype", cases(SC.VIT))
def test_vit_assemble_emulation_within_bounds(name, dtype):
    c = SC.VIT_BY[name]
    patch, cls, pos = SC.vit_inputs(c, dtype)
    ref, bound = SR.vit_assemble_ref(patch, cls, pos, c["B"], c["S"], dtype)
    check(SR.emu_vit_assemble(patch, cls, pos, c["B"], c["S"], dtype), ref, bound, f"vit_assemble/{dtype} x: {name}")


@pytest.mark.parametrize("name,dtype", cases(SC.VIT_BWD))
def test_vit_assemble_bwd_emulation_within_bounds(name, dtype):
    c = SC.VIT_BWD_BY[name]
    dx, dpos0, dcls0 = SC.vit_bwd_inputs(c, dtype)
    r_dp, (r_pos, e_pos), (r_cls, e_cls) = SR.vit_bwd_ref(dx, dpos0, dcls0, SC.vit_bwd_k(c, dtype))
    dp, dpos, dcls = SR.emu_vit_bwd(dx, dpos0, dcls0, SC.vit_bwd_slices(c, dtype))
    assert np.array_equal(dp, r_dp)
    check(dpos, r_pos, e_pos, f"vit_assemble_bwd/{dtype} dpos: {name}")
    check(dcls, r_cls, e_cls, f"vit_assemble_bwd/{dtype} dcls: {name}")


@pytest.mark.parametrize("name,dtype", cases(SC.EMBED_FWD[:3]))
def test_embed_fwd_emulation_within_bounds(name, dtype):
    """the product and the sum rounded separately, and as one contracted operation: the bound holds either way"""
    c = SC.EMBED_FWD_BY[name]
    ids, pos, table, ptab = SC.embed_fwd_inputs(c, dtype)
    ref, bound = SR.embed_fwd_ref(ids, pos, table, ptab, SC.EMBED_SCALE, dtype)
    for contract in (False, True):
        check(SR.emu_embed_fwd(ids, pos, table, ptab, SC.EMBED_SCALE, dtype, contract), ref, bound, f"embed_fwd/{dtype} h: {name}")


@pytest.mark.parametrize("name,dtype", cases(SC.EMBED_BWD))
def test_embed_bwd_emulation_within_bounds(name, dtype):
    c = SC.EMBED_BWD_BY[name]
    ids, pos, dh, dt0, dp0 = SC.embed_bwd_inputs(c, dtype)
    (r_t, e_t), (r_p, e_p) = SR.embed_bwd_ref(ids, pos, dh, SC.EMBED_SCALE, c["V"], c["P"] + 2, dt0, dp0)
    dt, dp = SR.emu_embed_bwd(ids, pos, dh, SC.EMBED_SCALE, c["V"], c["P"] + 2, dt0, dp0)
    check(dt, r_t, e_t, f"embed_bwd/{dtype} dtable: {name}")
    check(dp, r_p, e_p, f"embed_bwd/{dtype} dpos_table: {name}")
    assert (np.bincount(ids) >= c["rows"] // 3).any()


@pytest.mark.parametrize("name,dtype", cases(SC.DET))
def test_det_emulation_within_bounds(name, dtype):
    """the documented tree in fp32 lies within the fp64 bound with scale 0.37 (where the emulation rounds t * scale and the add
    separately; the kernel may contract them: both are within the bound)"""
    c = SC.DET_BY[name]
    ids, _ = SC.det_ids(c)
    dh, base = SC.det_inputs(c, dtype)
    ref, bound = SR.det_ref(ids, np.nan_to_num(dh), 0.37, base)
    check(SR.emu_det(ids, dh, 0.37, base), ref, bound, f"embed_rows_add_det/{dtype} dtable scale 0.37: {name}")


@pytest.mark.parametrize("name,dtype", cases(SC.COLSUM))
def test_colsum_emulation_within_bounds(name, dtype):
    c = SC.COLSUM_BY[name]
    x, start = SC.colsum_inputs(c["rows"], c["cols"], dtype)
    plan = SC.colsum_plan(c["rows"], c["cols"])
    st = start if c["acc"] else None
    ref, bound = SR.colsum_ref(x, plan[3], st)
    check(SR.emu_colsum(x, plan, st), ref, bound, f"colsum/{dtype} out: {name}")


@pytest.mark.parametrize("scale_inv", SC.Q8_SCALES)
@pytest.mark.parametrize("fmt", SC.Q8_FMTS)
@pytest.mark.parametrize("name", [c["name"] for c in SC.COLSUM_Q8])
def test_colsum_q8_emulation_within_bounds(name, fmt, scale_inv):
    c = SC.COLSUM_Q8_BY[name]
    b = SC.q8_bytes(c["rows"], c["cols"], fmt)
    plan = SC.colsum_plan(c["rows"], c["cols"])
    start = SC.start_values(np.random.default_rng(c["rows"] + c["cols"]), np.abs(SR.q8_decode(b, fmt)).sum(0) * scale_inv)
    ref, bound = SR.colsum_q8_ref(b, fmt, scale_inv, plan[3], start)
    check(SR.emu_colsum(SR.q8_decode(b, fmt), plan, start, scale=scale_inv), ref, bound, f"colsum_q8/f32 out {fmt}: {name} scale_inv {scale_inv}")


def test_fp8_tables_against_the_format_definitions():
    """landmarks of the OCP formats; with torch at hand, the whole table against its CPU cast (a cross-check, not the reference)"""
    e4, e5 = SR.Q8_TABLE["e4m3"], SR.Q8_TABLE["e5m2"]
    assert e4[0x7E] == 448 and e4[0x08] == 2.0 ** -6 and e4[0x01] == 2.0 ** -9 and np.isnan(e4[0x7F]) and np.isnan(e4[0xFF]) and e4[0x38] == 1
    assert e5[0x7B] == 57344 and e5[0x04] == 2.0 ** -14 and e5[0x01] == 2.0 ** -16 and np.isposinf(e5[0x7C]) and np.isnan(e5[0x7D]) and e5[0x3C] == 1
    assert np.signbit(e4[0x80]) and e4[0x80] == 0 and np.isfinite(e4).sum() == 254 and np.isfinite(e5).sum() == 248
    try:
        import torch
    except ImportError:
        torch = None
    for fmt, td in (("e4m3", "float8_e4m3fn"), ("e5m2", "float8_e5m2")) if torch is not None else ():
        t = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(getattr(torch, td)).float().double().numpy()
        assert np.array_equal(t, SR.Q8_TABLE[fmt], equal_nan=True)
    for fmt in SC.Q8_FMTS:  # the operands hold every finite byte, and a column of subnormals and zeros
        b = SC.q8_bytes(520, 8, fmt)
        assert set(np.flatnonzero(np.isfinite(SR.Q8_TABLE[fmt]))) <= set(b.reshape(-1).tolist())
        assert (np.abs(SR.q8_decode(b[:, 1], fmt)) < (2.0 ** -6 if fmt == "e4m3" else 2.0 ** -14)).all() and SR.q8_decode(b[:, 1], fmt).any()


@pytest.mark.parametrize("dtype", SC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in SC.SLABS[:3]])
def test_sum_slabs_emulation_within_bounds(name, dtype):
    x = SC.slab_inputs(SC.SLABS_BY[name])
    ref, bound = SR.sum_slabs_ref(x, dtype)
    check(SR.emu_sum_slabs(x, dtype), ref, bound, f"sum_slabs/{dtype} dst: {name}")


@pytest.mark.parametrize("name", [c["name"] for c in SC.LABEL_TERMS])
def test_label_terms_emulation_within_bounds(name):
    labels, coef, E, h, dE0 = SC.label_terms_inputs(SC.LABEL_TERMS_BY[name])
    r_dx, e_dx, r_dE, e_dE = SR.label_terms_ref(labels, coef, E, h, dE0)
    dx, dE = SR.emu_label_terms(labels, coef, E, h, dE0)
    check(dx, r_dx, e_dx + 1e-300, f"head_label_terms/bf16 dx_slab: {name}")
    check(dE, r_dE, e_dE, f"head_label_terms/bf16 dE: {name}")
    assert (coef == 0).any() and (np.bincount(labels[coef != 0]) > 1).any()


def test_rne_to_bf16_on_the_special_operands():
    """the expected bits of the fp32 -> bf16 cast, pattern by pattern"""
    exp, nan = SR.cast_expected_bits(SC.CAST_SPECIAL, "f32", "bf16")
    want = [0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x3F81, 0x3F80, 0x7F7F, 0x7F80, 0xFF80, 0x0000, 0x0000, 0x0002, 0x0080, 0x8001, 0x0000, 0x8000,
            0x7F80, 0xFF80]
    assert exp[:18].tolist() == want and nan.tolist() == [False] * 18 + [True, True]
    assert len(SC.cast_split(SC.CAST_N[0])) == 2 and SC.cast_split(SC.CAST_N[1]) == [(2, 1 << 20), (1, 3)] and SC.cast_split(100) == [(1, 100)]


# ------------------------------------------------------------------------------------------------ seeded defects
DEFECTS = {}   # name -> (rejected by, old relerr, old threshold or None where the old test compares exactly)


def _record(name, by, bad=None, ref=None, dtype="f32", exact_before=False):
    DEFECTS[name] = (by, None if bad is None else old_relerr(bad, ref), None if exact_before else OLD_TOL[dtype])


def _det(name, dtype="bf16", scale=0.5):
    c = SC.DET_BY[name]
    ids, _ = SC.det_ids(c)
    dh, base = SC.det_inputs(c, dtype)
    ref, bound = SR.det_ref(ids, np.nan_to_num(dh), scale, base)
    return ids, dh, base, ref, bound, SR.emu_det(ids, dh, scale, base)


def test_defect_det_plain_mod16_grouping():
    """stays inside the fp64 bound: only the bitwise comparison with the documented order sees it (on fp32 rows: a few dozen bf16
    values add up exactly in fp32, in any order)"""
    ids, dh, base, ref, bound, good = _det("det_1100x1024", "f32")
    bad = SR.emu_det(ids, dh, 0.5, base, defect="mod16")
    check(bad, ref, bound, "mod16", log=False)
    assert not bits_equal(bad, good)
    _record("det: plain w % 16 grouping", "bitwise order", bad, ref)


DET_DEFECTS = [("single_twice", "det_13x1088", "det: last == first added twice on the count-2 path"),
               ("no_tail", "det_5x64", "det: scalar tail of the id scan (n % 4) skipped"),
               ("no_tail", "det_1102x1088", "det: scalar tail skipped, n 1102"),
               ("no_block2", "det_13x1088", "det: second 1024-column block skipped")]
COLSUM_DEFECTS = [("no_partial_chunk", "cs_7x204"), ("no_last_slice", "cs_65x264")]
FP8_DEFECTS = [("as_e4m3", "colsum_q8: e5m2 bytes decoded as e4m3"), ("flush_subnormals", "colsum_q8: fp8 subnormals flushed")]


@pytest.mark.parametrize("defect,name,label", DET_DEFECTS)
def test_defect_det(defect, name, label):
    ids, dh, base, ref, bound, good = _det(name)
    check(good, ref, bound, "det", log=False)
    bad = SR.emu_det(ids, dh, 0.5, base, defect=defect)
    rejected(bad, ref, bound, label)
    _record(label, "fp64 bound", bad, ref)


@pytest.mark.parametrize("defect,name", COLSUM_DEFECTS)
def test_defect_colsum(defect, name):
    c = SC.COLSUM_BY[name]
    x, _ = SC.colsum_inputs(c["rows"], c["cols"], "bf16")
    plan = SC.colsum_plan(c["rows"], c["cols"])
    ref, bound = SR.colsum_ref(x, plan[3])
    bad = SR.emu_colsum(x, plan, defect=defect)
    rejected(bad, ref, bound, defect)
    _record(f"colsum: {defect}", "fp64 bound", bad, ref)


def test_defects_vit_assemble_bwd():
    c = SC.VIT_BWD_BY["vitb_9x3x64"]
    dx, dpos0, dcls0 = SC.vit_bwd_inputs(c, "bf16")
    r_dp, _, (r_cls, e_cls) = SR.vit_bwd_ref(dx, dpos0, dcls0, SC.vit_bwd_k(c, "bf16"))
    dp, _, _ = SR.emu_vit_bwd(dx, dpos0, dcls0, 4, defect="dpatch_bS")
    assert not np.array_equal(dp, r_dp)
    _record("vit_assemble_bwd: dpatch indexed with b * S", "exact", exact_before=True)
    _, _, dcls = SR.emu_vit_bwd(dx, dpos0, dcls0, 4, defect="dcls_all_s")
    rejected(dcls, r_cls, e_cls, "dcls")
    _record("vit_assemble_bwd: dcls summed over all s", "fp64 bound", dcls, r_cls)
    patch, cls, pos = SC.vit_inputs(SC.VIT_BY["vit_2x50x12"], "bf16")
    ref, bound = SR.vit_assemble_ref(patch, cls, pos, 2, 50, "bf16")
    bad = SR.emu_vit_assemble(patch, cls, pos, 2, 50, "bf16", defect="patch_row_bS")
    rejected(bad, ref, bound, "x")
    _record("vit_assemble: patch row b * S", "fp64 bound", bad, ref, "bf16")


def test_defects_embedding():
    c = SC.EMBED_FWD_BY["emb_37x520"]
    ids, pos, table, ptab = SC.embed_fwd_inputs(c, "bf16")
    ref, bound = SR.embed_fwd_ref(ids, pos, table, ptab, SC.EMBED_SCALE, "bf16")
    bad = SR.emu_embed_fwd(ids, pos, table, ptab, SC.EMBED_SCALE, "bf16", defect="no_plus2")
    rejected(bad, ref, bound, "h")
    _record("embed_fwd: the + 2 of the position table missing", "fp64 bound (and NaN rows 0, 1)", bad, ref, "bf16")
    c = SC.EMBED_BWD_BY["embb_37x64"]
    ids, pos, dh, dt0, dp0 = SC.embed_bwd_inputs(c, "bf16")
    _, (r_p, e_p) = SR.embed_bwd_ref(ids, pos, dh, SC.EMBED_SCALE, c["V"], c["P"] + 2, dt0, dp0)
    _, bad = SR.emu_embed_bwd(ids, pos, dh, SC.EMBED_SCALE, c["V"], c["P"] + 2, dt0, dp0, defect="scale_on_dpos")
    rejected(bad, r_p, e_p, "dpos")
    _record("embed_bwd: scale applied to dpos", "fp64 bound", bad, r_p)


def test_defects_data_movement():
    sb = SC.cast_source_bits(165, "f32")
    good, nan = SR.cast_expected_bits(sb, "f32", "bf16")
    bad, _ = SR.cast_expected_bits(sb, "f32", "bf16", defect="truncate")
    assert not np.array_equal(good[~nan], bad[~nan])
    f = lambda b: (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)  # noqa: E731
    fin = ~nan & np.isfinite(f(good)) & np.isfinite(f(bad))
    _record("cast: truncation in place of RNE", "exact bits", f(bad)[fin], f(good)[fin], "bf16")
    c = SC.IM2COL_BY["i2c_2x24_p4"]
    px = SC.im2col_inputs(c)
    good, bad = (SR.im2col_ref(px, 2, 24, 4, 0, "bf16", defect=d) for d in (None, "k_order_cuv"))
    assert not np.array_equal(good, bad)
    _record("im2col: k order (c, u, v)", "exact", exact_before=True)
    x = SC.slab_inputs(SC.SLABS_BY["slab_7x5x24"])
    ref, bound = SR.sum_slabs_ref(x, "f32")
    bad = SR.emu_sum_slabs(x, "f32", defect="pairwise")
    check(bad, ref, bound, "pairwise", log=False)   # a legitimate sum in another order: only the bitwise check rejects it
    assert not bits_equal(bad, SR.emu_sum_slabs(x, "f32"))
    _record("sum_slabs: slabs summed pairwise", "bitwise order", bad, ref)


@pytest.mark.parametrize("defect,label", FP8_DEFECTS)
def test_defects_fp8_decode(defect, label):
    c = SC.COLSUM_Q8_BY["csq_520x8"]
    b = SC.q8_bytes(c["rows"], c["cols"], "e5m2")
    plan = SC.colsum_plan(c["rows"], c["cols"])
    start = np.zeros(c["cols"])
    ref, bound = SR.colsum_q8_ref(b, "e5m2", 0.25, plan[3], start)
    bad = SR.emu_colsum(SR.q8_decode(b, "e5m2", defect), plan, start, scale=0.25)
    rejected(bad, ref, bound, label)
    _record(label, "fp64 bound", bad, ref)


def test_defect_label_term_of_a_zero_coefficient():
    labels, coef, E, h, dE0 = SC.label_terms_inputs(SC.LABEL_TERMS_BY["hlt_5x8"])
    _, _, r_dE, e_dE = SR.label_terms_ref(labels, coef, E, h, dE0)
    _, bad = SR.emu_label_terms(labels, coef, E, h, dE0, defect="zero_coef_adds")
    rejected(bad, r_dE, e_dE, "dE")
    _record("head_label_terms: a coef == 0 row still adds", "fp64 bound", bad, r_dE)


def test_defects_the_old_tolerance_accepts():
    """prints, for every seeded defect above, whether relerr of tests/test_ops_gpu.py under its threshold accepts the defective
    result (no count is asserted: the list goes into the commit message)"""
    DEFECTS.clear()
    test_defect_det_plain_mod16_grouping()
    for a in DET_DEFECTS:
        test_defect_det(*a)
    for a in COLSUM_DEFECTS:
        test_defect_colsum(*a)
    for a in FP8_DEFECTS:
        test_defects_fp8_decode(*a)
    test_defects_vit_assemble_bwd()
    test_defects_embedding()
    test_defects_data_movement()
    test_defect_label_term_of_a_zero_coefficient()
    assert len(DEFECTS) >= 16
    for name, (by, rel, thr) in sorted(DEFECTS.items()):
        verdict = "compared exactly before" if thr is None else (f"old relerr {rel:.3g} < {thr:g}: ACCEPTED" if rel < thr else f"old relerr {rel:.3g} >= {thr:g}: rejected")
        print(f"[defect] {name}: new check rejects it by {by}; {verdict}")


# ------------------------------------------------------------------------------------------------ dispatch rules and coverage
def test_dispatch_rules_and_claims():
    vec = {c["name"]: SC.im2col_vec(c, "bf16") for c in SC.IM2COL}
    assert vec == {"i2c_2x64_p32": True, "i2c_1x48_p16": True, "i2c_2x24_p4": False, "i2c_1x48_p16_ldp4": False, "i2c_1x48_p16_base8": False,
                   "i2c_2x64_p32_trunc": True, "i2c_2x24_p4_trunc": False}
    sl = {c["name"]: (SC.vit_bwd_slices(c, "bf16"), SC.vit_bwd_slices(c, "f32")) for c in SC.VIT_BWD}
    assert sl == {"vitb_1x3x64": (1, 0), "vitb_9x3x64": (4, 0), "vitb_33x2x16": (8, 0), "vitb_2x50x768": (1, 0), "vitb_3x3x12": (0, 0),
                  "vitb_3x3x16_ldp4": (0, 0)}
    # the empty and the ragged slice
    assert -(-9 // 4) * 3 >= 9 and -(-33 // 8) * 6 < 33 <= -(-33 // 8) * 7
    assert [SC.colsum_plan(r, c) for r, c in ((1, 8), (7, 204), (64, 256), (65, 264), (8200, 2048))] == \
        [(1, 1, 1, 10), (1, 1, 7, 10), (1, 1, 64, 17), (2, 2, 33, 15), (8, 128, 65, 145)]
    assert len(SC.COLSUM_GROUP) == 9 == len(SC.COLSUM_Q8_GROUP) and all(c % 8 == 0 for _, c in SC.COLSUM_Q8_GROUP)
    # grid-stride trips: more work items than the launch has threads
    assert 7 * 50 * 768 > 1024 * 256 and 4100 * 128 > 2048 * 256 and 1030 * 1024 > 4096 * 256 and 2052 * 256 > 2048 * 256
    assert 2100 * 512 > 4096 * 256 and SC.DROPOUT_N > 1024 * 256
    for c in SC.DET:
        ids, planted = SC.det_ids(c)
        cnt = np.bincount(ids[ids >= 0])
        if c["n"] >= 64:
            assert {1, 2, 3, 4, 5, 9, 32} <= set(cnt.tolist()) and ids[0] != ids[-1] and cnt[0] == 3 and cnt[c["vocab"] - 1] == 2
            assert len({p >> 5 for p in planted[3]}) == 1 and len({p >> 5 for p in planted[c["vocab"] - 3]}) == len(planted[c["vocab"] - 3]) >= 33
        if c["n"] % 4:
            assert cnt[ids[-1]] > 2 or c["n"] == 1
        assert (c["neg"] == 0) == ((ids < 0).sum() == 0) and (not c["neg"] or (ids < 0).sum() >= c["n"] // 4)
    assert {c["n"] for c in SC.DET} >= {1, 5, 13, 1100, 65536} and {c["width"] for c in SC.DET} == {64, 1024, 1088, 2048}
    assert len(planted[c["vocab"] - 3]) == 40


def test_every_instantiation_in_scope_has_a_case_and_is_launched():
    ns = lambda names: {re.sub(r"\s+", "", n) for n in names}  # noqa: E731
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")))
    built = {k for unit in table.values() for k in unit if SC.IN_SCOPE.match(k)}
    assert len(built) >= 33
    assert ns(built) == ns(SC.claimed_kernels()), sorted(ns(built) ^ ns(SC.claimed_kernels()))
    with open(os.path.join(ROOT, COVERAGE_PROFILE)) as f:
        traced = ns(line[:100].strip() for line in f)
    assert ns(built) <= traced, sorted(ns(built) - traced)
