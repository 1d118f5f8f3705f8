"""The check on the checker of the row-op conformance suite; runs without a GPU.
  - fp32 numpy emulations of the kernels' arithmetic as written (util_rowop_ref.emu_*) lie within the derived bounds on every case
    of util_rowop_cases.py (the printed ratios are the emulation's column of profiles/rowop_conformance_worst_ratio.txt);
  - seeded defects, applied to the emulations, are rejected on a named case — and for three of them the old assertion of
    tests/test_ops_gpu.py (max-scaled relerr under tol(dtype)) is shown to accept the defective result;
  - every kernel instantiation in scope is claimed by a case, launched by the GPU module (its committed kernel listing) and covers
    the build's resource table and the product's committed profiles.
Out of scope (as in the GPU module): the _q8 forms (tests/test_fp8_conformance_{cpu,gpu}.py), embeddings / ViT assembly / colsum, the decode epilogues."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_rowop_cases as RC  # noqa: E402
import util_rowop_ref as RR  # noqa: E402
from util_gemm_ref import check, round_to  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_PROFILES = ("profiles/r6_train_kernel_stats_serial.txt", "profiles/r6_train_fp8_kernel_stats_serial.txt",
                    "profiles/r6_generate_kernel_stats.txt")
COVERAGE_PROFILE = "profiles/rowop_conformance_kernel_stats.txt"
Q8_KERNELS = ("ln_fwd_kernel<unsigned short, true>", "ln_bwd_kernel<unsigned short, 2, 8, 1>", "ln_bwd_kernel<unsigned short, 2, 8, 2>",
              "ln_bwd_kernel<unsigned short, 4, 8, 1>", "ln_bwd_kernel<unsigned short, 4, 8, 2>", "ce_bwd_q8_kernel")
OLD_TOL = {"f32": 2e-5, "bf16": 1.2e-2}   # tests/test_ops_gpu.py tol(dtype)


def old_relerr(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-6))


def rejected(got, ref, bound, what):
    with pytest.raises(AssertionError):
        check(got, ref, bound, what, log=False)


# ------------------------------------------------------------------------------------------------ emulations within the bounds
@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("p", RC.LN_DROPOUT)
@pytest.mark.parametrize("name", [c["name"] for c in RC.LN_FWD])
def test_ln_fwd_emulation_within_bounds(name, p, dtype):
    c = RC.LN_ALL[name]
    x, g, b, _, _ = RC.ln_inputs(c, dtype)
    keep = RR.keep_mask(x.size, p, 77)
    y, mean, rstd = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype, keep, p)
    f = RR.ln_fwd_ref(x, g, b, RC.LN_EPS, dtype, keep, p)
    check(mean, f["mean"], f["bound_mean"], f"ln_fwd/{dtype} mean: {name}")
    check(rstd, f["rstd"], f["bound_rstd"], f"ln_fwd/{dtype} rstd: {name}")
    check(y, f["y"], f["bound_y"], f"ln_fwd/{dtype} y: {name}")
    assert not y.reshape(-1)[~keep].any()


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in RC.LN_BWD])
def test_ln_bwd_emulation_within_bounds(name, dtype):
    c = RC.LN_ALL[name]
    fl = RC.LN_FLAGS[c["flags"]]
    x, g, b, dy, dres = RC.ln_inputs(c, dtype)
    _, mean, rstd = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype)
    kin = RR.keep_mask(x.size, 0.1, 5) if "in_dropout" in fl else None
    dr = dres if "dres" in fl else None
    dx, dg, db, part = RR.emu_ln_bwd(x, g, mean, rstd, dy, dtype, dres=dr, keep_in=kin, p_in=0.1, nblk=RC.ln_bwd_blocks(c["rows"]))
    r = RR.ln_bwd_ref(x, g, mean, rstd, dy, dtype, dres=dr, keep_in=kin, p_in=0.1)
    check(dx, r["dx"], r["bound_dx"], f"ln_bwd/{dtype} dx: {name}")
    check(dg, r["dgamma"], r["bound_dgamma"], f"ln_bwd/{dtype} dgamma: {name}")
    check(db, r["dbeta"], r["bound_dbeta"], f"ln_bwd/{dtype} dbeta: {name}")
    check(part[0].astype(np.float64).sum(0), r["dgamma"], r["bound_dgamma"], f"ln_bwd/{dtype} partials dgamma: {name}")
    if c["rows"] <= 50:
        f = RR.ln_fwd_ref(x, g, b, RC.LN_EPS, dtype)
        e = RR.ln_bwd_ref(x, g, f["mean"], f["rstd"], dy, dtype, dres=dr, keep_in=kin, p_in=0.1, fwd=f)
        check(dx, e["dx"], e["bound_dx"], f"ln_bwd/{dtype} dx end to end: {name}")
        check(dg, e["dgamma"], e["bound_dgamma"], f"ln_bwd/{dtype} dgamma end to end: {name}")


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("ls", RC.CE_LS)
@pytest.mark.parametrize("name", [c["name"] for c in RC.CE])
def test_ce_emulation_within_bounds(name, ls, dtype):
    c = RC.CE_BY[name]
    x, labels, mask = RC.ce_inputs(c, dtype)
    lse, loss = RR.emu_ce_rows(x, labels, ls)
    r = RR.ce_rows_ref(x, labels, ls)
    check(lse, r["lse"], r["bound_lse"], f"ce_rows/{dtype} row_lse: {name}")
    if c.get("neginf") and ls > 0:  # the smoothed loss of a row with a -inf logit is +inf, in the reference and in the kernel
        inf = np.isinf(x).any(1)
        assert np.array_equal(np.isposinf(loss), inf) and np.array_equal(np.isposinf(r["loss"]), inf)
        loss, r = loss[~inf], {k: v[~inf] for k, v in r.items()}
    check(loss, r["loss"], r["bound_loss"], f"ce_rows/{dtype} row_loss ls={ls}: {name}")
    den = float(mask.sum())
    xp = np.zeros((c["rows"], c["Vpad"]))
    xp[:, :c["V"]] = x
    got = RR.emu_ce_bwd(xp, c["V"], labels, mask, ls, lse, den, 4.0, dtype)
    v, e = RR.ce_bwd_ref(xp, c["V"], labels, mask, ls, lse, den, 4.0, dtype)
    check(got, v, e, f"ce_bwd/{dtype} dlogits ls={ls}: {name}")


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_ce_neginf_chunk_old_loop_gives_nan_new_loop_is_finite(dtype):
    """the loop without the guard forms exp(-inf - -inf) on a chunk of -inf under a running maximum of -inf.  ce_1003_neginf_chunk:
    with 126 chunks every such thread first merges with an absent thread in the LDS tree, whose guard resets the NaN sum to 0 — the
    result is right by luck.  ce_2100_neginf_chunk: thread 0 has a second chunk and a present partner, the NaN reaches row_lse.
    With the guard the emulation meets the reference on every row of both."""
    for name, nan_rows in (("ce_1003_neginf_chunk", []), ("ce_2100_neginf_chunk", [1, 2, 3, 5, 6, 7])):
        x, labels, _ = RC.ce_inputs(RC.CE_BY[name], dtype)
        old, _ = RR.emu_ce_rows(x, labels, 0.0, guard=False)
        assert np.flatnonzero(np.isnan(old)).tolist() == nan_rows, name
        new, _ = RR.emu_ce_rows(x, labels, 0.0)
        r = RR.ce_rows_ref(x, labels, 0.0)
        assert np.isfinite(r["lse"]).all()
        check(new, r["lse"], r["bound_lse"], "ce_rows row_lse", log=False)


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("V", RC.CE_TILES)
def test_ce_tiles_emulation_within_bounds(V, dtype):
    rng = np.random.default_rng(V)
    x = round_to(rng.standard_normal((6, V)) * 3, dtype)
    x[1, 64:128] = -np.inf
    labels = RC.ce_labels(6, V)
    labels[1] = 3
    part = RR.tile_partials(x)
    assert part[1, 1, 0] == -np.inf and part[1, 1, 1] == 0
    xl = x[np.arange(6), labels]
    r = RR.ce_tiles_ref(part, xl)
    full = RR.ce_rows_ref(x, labels, 0.0)
    assert np.abs(r["lse"] - full["lse"]).max() < 1e-5
    for aligned in (True, False):
        lse, loss = RR.emu_ce_tiles(part, xl, aligned)
        check(lse, r["lse"], r["bound_lse"], f"ce_rows_tiles/{dtype} row_lse: V={V} {'aligned' if aligned else 'odd_ld'}")
        check(loss, r["loss"], r["bound_loss"], f"ce_rows_tiles/{dtype} row_loss: V={V} {'aligned' if aligned else 'odd_ld'}")


@pytest.mark.parametrize("name", [c["name"] for c in RC.ADAMW])
def test_adamw_emulation_within_bounds(name):
    c = RC.ADAMW_BY[name]
    p, m, v, g = RC.adamw_inputs(c, min(c["n"], 4100))
    h = RC.adamw_hyper(c)
    got = RR.emu_adamw(p, m, v, g, **h)
    r = RR.adamw_ref(p, m, v, g, **h)
    for a, k in zip(got, "pmv"):
        assert np.isfinite(a).all()
        check(a, r[k], r["bound_" + k], f"adamw/f32 {k}: {name}")
    if c["lr"] == 0:
        assert np.array_equal(got[0], p.astype(np.float32))


# ------------------------------------------------------------------------------------------------ seeded defects
def _ln_case(name, dtype):
    c = RC.LN_ALL[name]
    x, g, b, dy, dres = RC.ln_inputs(c, dtype)
    return c, x, g, b, dy, dres


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_one_pass_variance_is_caught_by_rstd(dtype):
    """ln_9x768_shift: rows of mean LN_SHIFT, std 1.  The two-pass emulation stays under 0.5 of the rstd bound, E[x^2] - E[x]^2 leaves
    it — while y under the OLD tolerance accepts the defect"""
    c, x, g, b, _, _ = _ln_case("ln_9x768_shift", dtype)
    f = RR.ln_fwd_ref(x, g, b, RC.LN_EPS, dtype)
    y, _, rstd = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype)
    assert check(rstd, f["rstd"], f["bound_rstd"], "rstd", log=False) < 0.5
    yd, _, bad = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype, defect="one_pass")
    rejected(bad, f["rstd"], f["bound_rstd"], "rstd")
    if dtype == "bf16":  # the old assertion on y accepts it
        assert old_relerr(yd, round_to(f["y"], dtype)) < OLD_TOL[dtype]


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("defect", ["w_minus_1", "eps_outside"])
def test_ln_statistics_defects(defect, dtype):
    """ln_9x768 (variance over W - 1: the ordinary rows) / the constant and std-1e-3 rows (eps outside the square root)"""
    c, x, g, b, _, _ = _ln_case("ln_9x768", dtype)
    f = RR.ln_fwd_ref(x, g, b, RC.LN_EPS, dtype)
    _, _, bad = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype, defect=defect)
    rejected(bad, f["rstd"], f["bound_rstd"], "rstd")


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_ln_dropout_without_scale(dtype):
    c, x, g, b, _, _ = _ln_case("ln_9x768", dtype)
    keep = RR.keep_mask(x.size, 0.1, 77)
    f = RR.ln_fwd_ref(x, g, b, RC.LN_EPS, dtype, keep, 0.1)
    bad, _, _ = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype, keep, 0.1, defect="no_scale")
    rejected(bad, f["y"], f["bound_y"], "y")


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("defect,name", [("no_dres", "lnb_9x768"), ("no_c2_last", "lnb_3x520"), ("no_c2_last", "lnb_9x1032")])
def test_ln_bwd_dx_defects(defect, name, dtype):
    c, x, g, b, dy, dres = _ln_case(name, dtype)
    _, mean, rstd = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype)
    dr = dres if defect == "no_dres" else None
    r = RR.ln_bwd_ref(x, g, mean, rstd, dy, dtype, dres=dr)
    bad = RR.emu_ln_bwd(x, g, mean, rstd, dy, dtype, dres=dr, defect=defect)[0]
    rejected(bad, r["dx"], r["bound_dx"], "dx")
    if defect == "no_c2_last" and dtype == "bf16":  # one chunk of 8 columns in 520: the old max-scaled assertion accepts it
        assert old_relerr(bad, round_to(r["dx"], dtype)) < OLD_TOL[dtype]


@pytest.mark.parametrize("dtype", RC.DTYPES)
def test_ln_bwd_dgamma_registers_not_carried(dtype):
    """lnb_4107x64: 11 rows take the second grid-stride trip; dropping the first trip's registers of those waves"""
    c, x, g, b, dy, _ = _ln_case("lnb_4107x64", dtype)
    _, mean, rstd = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, dtype)
    r = RR.ln_bwd_ref(x, g, mean, rstd, dy, dtype)
    _, bad, _, _ = RR.emu_ln_bwd(x, g, mean, rstd, dy, dtype, nblk=512, defect="no_carry")
    rejected(bad, r["dgamma"], r["bound_dgamma"], "dgamma")


def _ce_case(name, dtype, extra_col=False):
    c = RC.CE_BY[name]
    x, labels, mask = RC.ce_inputs(c, dtype)
    return c, x, labels, mask


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("defect", ["pad_in_sum", "low_over_v", "no_norm"])
def test_ce_rows_defects(defect, dtype):
    """ce_1003 (a padded column in the row sum; the smoothing constant omitted), ce_9 (low = ls / V: visible at a small V)"""
    c, x, labels, _ = _ce_case("ce_9" if defect == "low_over_v" else "ce_1003", dtype)
    r = RR.ce_rows_ref(x, labels, 0.1)
    xe = np.concatenate([x, np.full((x.shape[0], 1), 2.0)], 1) if defect == "pad_in_sum" else x
    _, bad = RR.emu_ce_rows(xe, labels, 0.1, defect=defect)
    rejected(bad, r["loss"], r["bound_loss"], "row_loss")
    if defect == "pad_in_sum":  # one more logit of 2.0 under low = 1e-4: the old assertion accepts it
        assert old_relerr(bad, r["loss"]) < OLD_TOL[dtype]


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("defect", ["label_late", "masked_grad"])
def test_ce_bwd_defects(defect, dtype):
    c, x, labels, mask = _ce_case("ce_1003", dtype)
    lse = RR.ce_rows_ref(x, labels, 0.0)["lse"]
    xp = np.zeros((c["rows"], c["Vpad"]))
    xp[:, :c["V"]] = x
    v, e = RR.ce_bwd_ref(xp, c["V"], labels, mask, 0.1, lse, float(mask.sum()), 1.0, dtype)
    bad = RR.emu_ce_bwd(xp, c["V"], labels, mask, 0.1, lse, float(mask.sum()), 1.0, dtype, defect=defect)
    assert (labels[mask != 0] % 8 == 7).any()
    rejected(bad, v, e, "dlogits")


def test_dlogits_t_without_zero_padding():
    """cet_37: the exact check the GPU module applies to dlogits_t accepts the transpose and rejects one that leaves columns
    rows .. rows_pad as they were"""
    rng = np.random.default_rng(37)
    src = rng.integers(0, 0x7F00, size=(37, 520)).astype(np.uint16)
    RR.check_transposed(RR.emu_transpose(src, 64, 72), src, 37, 64)
    with pytest.raises(AssertionError):
        RR.check_transposed(RR.emu_transpose(src, 64, 72, defect="no_pad"), src, 37, 64)


@pytest.mark.parametrize("defect", ["t_minus_1", "eps_inside", "coupled_wd", "omb2_f32"])
def test_adamw_defects(defect):
    """adamw_4100_t7 (eps inside the square root: the same case with moments and gradients of the size of eps, where the two forms
    differ); (1 - b2) formed in fp32 is 3e-5 off and is rejected by the bound on v"""
    c = RC.ADAMW_BY["adamw_4100_t7"]
    p, m, v, g = RC.adamw_inputs(c)
    if defect == "eps_inside":
        m, v, g = m * 1e-6, v * 1e-12, g * 1e-6
    h = RC.adamw_hyper(c)
    r = RR.adamw_ref(p, m, v, g, **h)
    for a, k in zip(RR.emu_adamw(p, m, v, g, **h), "pmv"):
        check(a, r[k], r["bound_" + k], k, log=False)
    bad = RR.emu_adamw(p, m, v, g, defect=defect, **h)
    k = {"omb2_f32": "v"}.get(defect, "p")
    rejected(bad["pmv".index(k)], r[k], r["bound_" + k], k)


# ------------------------------------------------------------------------------------------------ coverage
def test_cases_meet_the_issue_floor():
    assert {c["width"] for c in RC.LN_FWD} >= {8, 520, 768, 1024, 1032, 2048} <= {c["width"] for c in RC.LN_BWD} | {8}
    assert {c["rows"] for c in RC.LN_FWD + RC.LN_BWD} >= {1, 3, 9, 50, 4107}
    assert {(c["rows"], c["width"]) for c in RC.LN_BWD} >= {(4107, 64), (4107, 1032)} and RC.ln_bwd_blocks(4107) * RC.LNB_WAVES < 4107
    assert {c["flags"] for c in RC.LN_BWD} >= {"none", "dres", "dxm", "dres_dxm", "in_dropout"}
    assert {(c["rows"], c["V"], c["Vpad"], c["ld"]) for c in RC.CE} >= {(24, 1003, 1024, 1024), (5, 9, 16, 24), (70, 8200, 8200, 8208),
                                                                       (300, 600, 640, 640), (3, 250054, 250112, 250112)}
    assert {-(-V // 64) % 4 for V in RC.CE_TILES} == {0, 1, 2, 3} and max(-(-V // 64) for V in RC.CE_TILES) > 256
    assert {c["mask"] for c in RC.CE} == {"ones", "one", "alt"}
    assert {c["n"] for c in RC.ADAMW} >= {4, 4100, 8388612} and {c["t"] for c in RC.ADAMW} >= {1, 7, 100000}
    assert {w for _, w in RC.ADAMW_ROWS} == {12, 1024, 1028, 2048}
    lab = RC.ce_labels(24, 1003)
    assert {0, 1002, 7, 8} <= set(lab.tolist())


def test_every_case_claims_a_kernel_in_scope():
    ns = lambda k: re.sub(r"\s+", "", k)  # noqa: E731
    claimed = {ns(k) for c in RC.LN_FWD + RC.LN_BWD for dt in RC.DTYPES for k in RC.ln_kernels_of(c, dt)}
    claimed |= {ns(k) for dt in RC.DTYPES for k in RC.ce_kernels_of(dt)}
    assert claimed <= {ns(k) for k in RC.KERNELS}
    assert {ns(k) for k in RC.KERNELS if k.startswith(("ln_fwd", "ln_bwd", "ce_rows_kernel", "ce_bwd", "ce_reduce"))} <= claimed
    for c in RC.LN_BWD:  # the dispatch rule restated: width <= 1024 runs the two-chunk build
        assert RC.ln_kernels_of(c, "f32") == [f"ln_bwd_kernel<float,{2 if c['width'] <= 1024 else 4},8,0>"]


def _instantiations(path):
    pat = r"\b(?:ln_[a-z_]*kernel|ce_[a-z_0-9]*kernel|adamw_kernel|tile_transpose_kernel)(?:<[^>]*>)?"
    with open(os.path.join(ROOT, path)) as f:
        return {re.sub(r"\s+", "", m) for m in re.findall(pat, f.read())}


def test_coverage_of_the_build_and_the_product_profiles():
    """the GPU module's committed kernel listing launches every instantiation in scope; the build's resource table and the product's
    committed profiles hold no LayerNorm / CE / AdamW / transpose instantiation beyond those and the fp8-emitting forms, which
    tests/test_fp8_conformance_gpu.py checks against fp64 and an fp8 reference of its own"""
    ns = lambda names: {re.sub(r"\s+", "", n) for n in names}  # noqa: E731
    traced = _instantiations(COVERAGE_PROFILE)
    assert ns(RC.KERNELS) <= traced, sorted(ns(RC.KERNELS) - traced)
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")))
    built = ns(k for unit in table.values() for k in unit if re.match(r"ln_|ce_|adamw_kernel|tile_transpose", k))
    assert len(built) >= 26
    assert built - ns(Q8_KERNELS) == ns(RC.KERNELS), sorted(built - ns(Q8_KERNELS) ^ ns(RC.KERNELS))
    prod = set().union(*(_instantiations(p) for p in PRODUCT_PROFILES))
    assert len(prod) >= 10
    assert prod - ns(Q8_KERNELS) <= traced, sorted(prod - traced)
