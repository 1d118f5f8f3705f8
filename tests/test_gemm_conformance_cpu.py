"""The GEMM conformance suite's own checks, on a machine without a GPU:
  - the element-wise checker of tests/util_gemm_ref.py bites: synthetic "kernel outputs" carrying the defects the old max-scaled
    tolerance let through are rejected, and the correctly rounded reference (and its fp32-accumulated twin) is accepted;
  - every case of tests/util_gemm_cases.py still gets, from the host planner (mic_gemm_plan: no device needed), the plan it claims;
  - the committed coverage profile of the GPU module names every GEMM instantiation of the product's committed profiles."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import util_gemm_cases as GC  # noqa: E402
import util_gemm_ref as GR  # noqa: E402

PRODUCT_PROFILES = ("profiles/r6_train_kernel_stats_serial.txt", "profiles/r6_train_fp8_kernel_stats_serial.txt",
                    "profiles/r6_generate_kernel_stats.txt")
COVERAGE_PROFILE = "profiles/gemm_conformance_kernel_stats.txt"


def _operands(M, N, K, seed=0):
    rng = np.random.default_rng(seed)
    A = GR.round_bf16(rng.standard_normal((M, K)))
    B = GR.round_bf16(rng.standard_normal((K, N)))
    return rng, A, B


def _fp32_epilogue(A, B, bias=None, alpha=1.0, act=0, R=None, keep=None, p=0.0):
    """what a correct kernel computes: fp32 accumulation (k-ordered), the epilogue in fp32, act on the rounded Z, bf16 store"""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    for k in range(A.shape[1]):
        acc = acc + np.outer(A32[:, k], B32[k]).astype(np.float32)
    v = acc * np.float32(alpha)
    if bias is not None:
        v = v + bias.astype(np.float32)[None, :]
    z = GR.round_bf16(v)
    if act:
        v = GR.act_fwd(act, z).astype(np.float32)
    if keep is not None:
        v = np.where(keep, v * np.float32(1.0 / (1.0 - p)), np.float32(0.0)).astype(np.float32)
    if R is not None:
        v = v + R.astype(np.float32)
    return GR.round_bf16(v), z


def test_checker_accepts_correct_rounding():
    M, N, K = 96, 72, 256
    rng, A, B = _operands(M, N, K)
    bias = rng.standard_normal(N)
    R = GR.round_bf16(4 * rng.standard_normal((M, N)))
    keep = rng.random((M, N)) >= 0.1
    ref = GR.gemm_ref(A, B, alpha=0.375, bias=bias, act=2, keep=keep, drop_p=0.1, R=R)
    GR.check(GR.round_bf16(ref["C"]), ref["C"], ref["bound_C"], "correctly rounded reference")
    got, z = _fp32_epilogue(A, B, bias, 0.375, 2, R, keep, 0.1)
    GR.check(got, ref["C"], ref["bound_C"], "fp32-accumulated epilogue")
    GR.check(z, ref["Z"], ref["bound_Z"], "fp32-accumulated Zout")
    # with the stored Z handed to the reference (the GPU module does that whenever Zout exists), the act branch is exact up to eps_f
    ref_z = GR.gemm_ref(A, B, alpha=0.375, bias=bias, act=2, z_stored=z, keep=keep, drop_p=0.1, R=R)
    GR.check(got, ref_z["C"], ref_z["bound_C"], "fp32-accumulated epilogue on the stored Z")
    # the bf16 unit roundoff is 2^-8: a round-half-even tie moves x by exactly 2^-8 |x|
    t = np.array([[1.0 + 2.0 ** -8]])
    GR.check(GR.round_bf16(t), t, GR.UBF16 * np.abs(t), "tie")


def _rejects(got, ref, bound, what):
    with pytest.raises(AssertionError):
        GR.check(got, ref, bound, what)


def test_checker_rejects_bias_missing_on_the_last_8_columns():
    M, N, K = 128, 136, 1024
    rng, A, B = _operands(M, N, K, 1)
    bias = 0.4 * rng.standard_normal(N)
    ref = GR.gemm_ref(A, B, bias=bias)
    got = GR.round_bf16(ref["C"] - np.where(np.arange(N) >= N - 8, bias, 0.0)[None, :])
    _rejects(got, ref["C"], ref["bound_C"], "bias missing on the last 8 columns")
    # ... which the max-scaled tolerance of the per-kernel tests (1.2e-2 of the largest output) does not notice
    assert np.abs(got - ref["C"]).max() / np.abs(ref["C"]).max() < 1.2e-2


def test_checker_rejects_alpha_ignored():
    rng, A, B = _operands(64, 64, 256, 2)
    ref = GR.gemm_ref(A, B, alpha=0.875)
    _rejects(GR.round_bf16(ref["C"] / 0.875), ref["C"], ref["bound_C"], "alpha ignored")


def test_checker_rejects_a_stale_row_behind_k_valid():
    K, kv = 320, 300
    rng, A, B = _operands(128, 64, K, 3)
    ref = GR.gemm_ref(A, B, k_valid=kv)
    leak = np.outer(A[:, kv], B[kv])  # one stale row (finite garbage) counted in dW
    _rejects(ref["C"] + leak, ref["C"], ref["bound_C"], "stale row in dW")
    s, b = GR.rowsum_ref(A[:, :kv])
    _rejects(s + A[:, kv], s, b, "stale row in a_rowsum")


def test_checker_rejects_dropout_scale_on_the_residual():
    M, N, K = 128, 128, 256
    rng, A, B = _operands(M, N, K, 4)
    R = GR.round_bf16(4 * rng.standard_normal((M, N)))
    keep = rng.random((M, N)) >= 0.1
    ref = GR.gemm_ref(A, B, keep=keep, drop_p=0.1, R=R)
    got = GR.round_bf16(ref["C"] + np.where(keep, R * (1 / 0.9 - 1), -R))
    _rejects(got, ref["C"], ref["bound_C"], "dropout applied to the residual")


def test_checker_rejects_act_before_rounding_z():
    """a Z in [1.5, 2) where GELU(Z) lies close to a bf16 value, and the unrounded pre-activation 0.49 ulp above it: GELU's slope
    > 1 moves the output over a rounding boundary.  The GPU module hands the kernel's stored Z to the reference, so the output
    bound has no room for a second rounding of Z."""
    zs = GR.round_bf16(np.linspace(1.5, 2.0, 4096, endpoint=False))
    zs = np.unique(zs)
    a = GR.act_fwd(1, zs)
    dist = np.abs(a - GR.round_bf16(a)) / 2.0 ** -7
    z = zs[np.argmin(dist)]
    z32 = np.float32(z + 0.49 * 2.0 ** -7)
    bad = GR.round_bf16(GR.act_fwd(1, np.float64(z32)))
    good = GR.round_bf16(GR.act_fwd(1, z))
    assert bad != good  # the case flips the result
    ref = GR.ref_epilogue(np.array([[z32]], np.float64), np.zeros((1, 1)), 64, act=1, z_stored=np.array([[z]]))
    GR.check(np.array([[good]]), ref["C"], ref["bound_C"], "act on the stored Z")
    _rejects(np.array([[bad]]), ref["C"], ref["bound_C"], "act applied before rounding Z")


def test_canary_sees_one_column_past_n():
    import torch

    M, N, ld = 16, 24, 32
    t = GR.sentinel_fill(torch.empty(M + 8, ld, dtype=torch.bfloat16))
    t[:M, :N] = 1.0
    GR.check_canary(t, (M, N))
    t[3, N] = 1.0
    with pytest.raises(AssertionError):
        GR.check_canary(t, (M, N))


def test_checker_rejects_nan_and_reports_ratio():
    ref = np.ones((4, 4))
    got = ref.copy()
    got[1, 2] = np.nan
    _rejects(got, ref, np.full_like(ref, 1e-3), "NaN")
    assert GR.check(ref, ref, np.full_like(ref, 1e-3), "exact") == 0.0


def test_sampling_covers_first_and_last_tiles():
    rng = np.random.default_rng(0)
    idx = GR.sample_idx(2404, rng)
    s = set(idx.tolist())
    for t in GR.TILE_HEIGHTS:
        assert set(range(t)) <= s and set(range((2403 // t) * t, 2404)) <= s
    assert len(idx) <= 2 * 256 + 64


@pytest.mark.parametrize("name", [c["name"] for c in GC.CASES])
def test_case_plan_claims(name):
    """each conformance case still gets, from the host planner, the plan (and so the kernel) it was written for"""
    c = GC.BY_NAME[name]
    from mic_amd import ops

    try:
        if c["cus"]:
            ops.set_cu_budget(c["cus"])
        rep = GC.plan_report(c)
        assert {k: rep[k] for k in c["plan"]} == c["plan"]
        # ... and the report names the instantiation the case claims (the launcher launches what the same decision says)
        assert GC.kernel_name(rep, c["dtype"], c["akm"], c["bkm"]) == c["kernel"], rep
    finally:
        ops.set_cu_budget(0)


def _instantiations(path):
    with open(os.path.join(ROOT, path)) as f:
        return {re.sub(r"\s+", "", m) for m in re.findall(r"gemm_[a-z0-9_]*kernel<[^>]*>", f.read())}


def test_coverage_of_the_product_profiles():
    """the GPU module's committed kernel trace launches every GEMM instantiation of the product's committed profiles"""
    prod = set().union(*(_instantiations(p) for p in PRODUCT_PROFILES))
    assert len(prod) >= 20
    missing = prod - _instantiations(COVERAGE_PROFILE)
    assert not missing, sorted(missing)
    assert all(c["kernel"] for c in GC.CASES)
    claimed = {re.sub(r"\s+", "", c["kernel"]) for c in GC.CASES}
    assert claimed <= _instantiations(COVERAGE_PROFILE), sorted(claimed - _instantiations(COVERAGE_PROFILE))
