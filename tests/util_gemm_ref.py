"""fp64 reference of the mic_gemm contract (include/mic_hip.h, mic_gemm_args) and an element-wise checker for the GEMM
conformance suite (tests/test_gemm_conformance_{cpu,gpu}.py).  A helper module, not a conftest.

The reference follows the header, not the kernels:

    v = acc * alpha + bias;  Zout = v;  v = act(Zout as stored);  v *= act'(Zin);  v = dropout(v; index m * N + n);
    v += R;  v += C_old;  C = round(v)

acc = op(A) op(B) over the full K (rows k >= k_valid of both operands count as zero).  fp8 operands enter dequantised:
acc * a_scale_inv * b_scale_inv.

Error bound (`ref_epilogue` carries it along the same steps; every quantity is per element):

    e_acc  = gamma_K * (|A| |B|)_mn,  gamma_K = 2 K 2^-24       (fp32 accumulation of exact products; bf16 x bf16 and
                                                                fp8 x fp8 products are exact in fp32, so only the K
                                                                additions round: |err| <= K u |A||B| to first order,
                                                                doubled for the split-K / K-group partial-sum merges)
    alpha  e = |alpha| e + u32 |v|                              (fp8: alpha * sa * sb, three roundings)
    bias   e = e + u32 |v|
    Zout   |Z - z| <= u_z |z| + (1 + u_z) e                     (the stored pre-activation)
    act    with the kernel's stored Z at hand the reference applies act to THAT z: e = eps_f (|z| + |act(z)|);
           without it: e = S_act (e + 2 u_z (|z| + e)) + eps_f (|z| + |act(z)|), S_act = 1.13 = max |gelu'| (the kernel's
           rounded z may differ from round(z) by one ulp)
    dact   e = |act'(Zin)| e + eps_f (1 + |Zin|)^2 |v| + u32 |v|
    drop   e = keep * scale * e + 2 u32 |v|
    R, C_old   e = e + u32 |v|
    C      |C - v| <= u_c |v| + (1 + u_c) e

fp32 operands (gemm_f32_kernel, the parity mode; tests/test_gemm_f32_conformance_{cpu,gpu}.py): the products are no longer exact in
fp32.  The kernel forms acc by K multiply-adds in ascending k (v_mfma_f32_32x32x2_f32), each of which rounds once when it is fused,
so |err| <= K u |A||B| to first order and gamma_K = 2 K 2^-24 covers it with the same factor 2 (which also covers a multiply-add
that rounds the product and the sum separately: 2 K roundings).  C_GAMMA, EPS_F and U32 are as for the bf16 kernels; u_c = u_z =
2^-24 (c_dtype = z_dtype = "f32").  `emu_gemm` below restates that kernel contract in numpy fp32 (with a `defect=` switch: the
checker has to reject what it is there for) and `check_problem` is the one comparison both modules run.

u_c, u_z: the unit roundoff of the stored type, 2^-8 for bf16 (8 significant bits; round-to-nearest moves x by up to 2^-8 |x|,
e.g. 1 + 2^-8 -> 1), 2^-24 for fp32.  eps_f = 32 * 2^-24: the fp32 evaluation error of erf / exp2 / rcp in act and act'.

By-products:
    a_rowsum[m] = sum_{k < rowsum_k} A(m, k):   |err| <= gamma_K sum |A(m, k)|
    rowstat[m][g] = (max, sum exp(x - max)) over the STORED C row's columns [64 g, 64 g + 64) & [0, nvalid):  max exact,
                    sum within 64 * 4 * 2^-24 relative (exp2 with one rounding each, 64 adds)
    rowsum2[m] = (sum, sum of squares) * 2^20 of the STORED row, int64:  |err| <= 2^20 * 2 * 128 * 2^-24 * sum |x|^(1|2)
                    + N / 32  (fp32 sums over <= 128-column wave tiles, one round-to-integer per tile)
    folded LayerNorm: v = rstd (acc - mu g) + bias', mu = s1 2^-20 / d, rstd = (s2 2^-20 / d - mu^2 + eps)^-1/2 from the int64
                    stats as given:  e = rstd (gamma_K S + 3 u32 |mu g| + u32 |acc - mu g|) + |rstd (acc - mu g)| d_rstd
                    + u32 |v|,  d_rstd = u32 (E[x^2] + mu^2) / var + 4 u32 — the cancellation in E[x^2] - mu^2 and in
                    acc - mu g is what a row mean of several sigma exercises.
"""
from __future__ import annotations

import math

import numpy as np

U32 = 2.0 ** -24
UBF16 = 2.0 ** -8
EPS_F = 32 * U32
C_GAMMA = 2
S_ACT = 1.13
TILE_HEIGHTS = (64, 128, 192, 256)


def u_of(dtype: str) -> float:
    return {"bf16": UBF16, "f32": U32}[dtype]


def round_bf16(x) -> np.ndarray:
    """round-to-nearest-even of float64 values to bf16 (through fp32: the values here are exact in fp32 or are rounded once
    more by the reference's own arithmetic), returned as float64"""
    f = np.asarray(x, dtype=np.float64).astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    out = (b & 0xFFFFFFFF).astype(np.uint32).view(np.float32).astype(np.float64)
    return np.where(np.isfinite(f), out, f.astype(np.float64))


def round_to(x, dtype: str) -> np.ndarray:
    return round_bf16(x) if dtype == "bf16" else np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def gamma_k(K: int) -> float:
    return C_GAMMA * K * U32


def sample_idx(n: int, rng: np.random.Generator, n_random: int = 64, heights=TILE_HEIGHTS) -> np.ndarray:
    """all rows of the first and the last tile at every tile height, plus n_random random rows"""
    s = set()
    for t in heights:
        s.update(range(0, min(t, n)))
        s.update(range(((n - 1) // t) * t, n))
    s.update(rng.choice(n, size=min(n_random, n), replace=False).tolist())
    return np.array(sorted(s), dtype=np.int64)


def _erf(x):
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def act_fwd(act: int, x):
    x = np.asarray(x, np.float64)
    if act == 1:
        return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    if act == 2:
        return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    if act == 3:
        return x / (1.0 + np.exp(-1.702 * x))
    return x


def act_bwd(act: int, x):
    x = np.asarray(x, np.float64)
    if act == 1:
        return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if act == 2:
        c = math.sqrt(2.0 / math.pi)
        t = np.tanh(c * (x + 0.044715 * x ** 3))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3 * 0.044715 * x * x)
    if act == 3:
        s = 1.0 / (1.0 + np.exp(-1.702 * x))
        return s + 1.702 * x * s * (1.0 - s)
    return np.ones_like(x)


def ref_epilogue(acc, S, K, *, alpha=1.0, scale=1.0, bias=None, act=0, z_stored=None, zin=None, dact=0, keep=None, drop_p=0.0,
                 R=None, C_old=None, c_dtype="bf16", z_dtype="bf16", ln=None):
    """The documented epilogue on fp64 accumulators `acc` [m][n] with |A||B| = S [m][n] over K.  Returns a dict with
    'C' (fp64 value before the final rounding), 'bound_C', and with a pre-activation 'Z', 'bound_Z'.  `scale`: the fp8
    dequantisation a_scale_inv * b_scale_inv; `ln`: (mu [m], rstd [m], g [n], d_rstd [m]) of a folded LayerNorm (bias is bias')."""
    acc = np.asarray(acc, np.float64)
    e = gamma_k(K) * S
    al = (alpha if alpha != 0.0 else 1.0) * scale
    if ln is not None:
        mu, rstd, g, d_rstd = (np.asarray(t, np.float64) for t in ln)
        mg = mu[:, None] * g[None, :]
        d = acc - mg
        v = rstd[:, None] * d
        e = rstd[:, None] * (e + 3 * U32 * np.abs(mg) + U32 * np.abs(d)) + np.abs(v) * d_rstd[:, None]
    else:
        v = acc * al
        e = abs(al) * e + (3 if scale != 1.0 else 1) * U32 * np.abs(v)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)[None, :]
        e = e + U32 * np.abs(v)
    out = {}
    if act or z_stored is not None:
        out["Z"], out["bound_Z"] = v.copy(), u_of(z_dtype) * np.abs(v) + (1 + u_of(z_dtype)) * e
    if act:
        if z_stored is not None:
            z = np.asarray(z_stored, np.float64)
            v = act_fwd(act, z)
            e = EPS_F * (np.abs(z) + np.abs(v))
        else:
            z = round_to(v, z_dtype)
            ez = e + 2 * u_of(z_dtype) * (np.abs(v) + e)
            v = act_fwd(act, z)
            e = S_ACT * ez + EPS_F * (np.abs(z) + np.abs(v))
    if dact:
        zin = np.asarray(zin, np.float64)
        d = act_bwd(dact, zin)
        e = np.abs(d) * e + EPS_F * (1 + np.abs(zin)) ** 2 * np.abs(v)
        v = v * d
        e = e + U32 * np.abs(v)
    if keep is not None and drop_p > 0.0:
        sc = 1.0 / (1.0 - drop_p)
        k = np.asarray(keep, np.float64)
        v = v * sc * k
        e = e * sc * k + 2 * U32 * np.abs(v)
    if R is not None:
        v = v + np.asarray(R, np.float64)
        e = e + U32 * np.abs(v)
    if C_old is not None:
        v = v + np.asarray(C_old, np.float64)
        e = e + U32 * np.abs(v)
    out["C"], out["bound_C"] = v, u_of(c_dtype) * np.abs(v) + (1 + u_of(c_dtype)) * e
    return out


def gemm_ref(A, B, *, k_valid=0, **epi):
    """A [m][K] (rows of op(A)), B [K][n] (columns of op(B)), fp64 (bf16 / dequantised fp8 values); rows k >= k_valid of both
    count as zero.  Keyword arguments: those of ref_epilogue."""
    A = np.asarray(A, np.float64)
    B = np.asarray(B, np.float64)
    K = A.shape[1]
    if k_valid:
        A, B = A[:, :k_valid], B[:k_valid]
    return ref_epilogue(A @ B, np.abs(A) @ np.abs(B), K, **epi)


def rowsum_ref(A, rowsum_k=0):
    """a_rowsum of rows of op(A): (sum, bound)"""
    A = np.asarray(A, np.float64)
    K = A.shape[1]
    if rowsum_k:
        A = A[:, :rowsum_k]
    return A.sum(1), gamma_k(K) * np.abs(A).sum(1) + 1e-30


def rowstat_ref(C_rows, nvalid):
    """(max, sum exp(x - max)) per 64-column granule of the stored rows C_rows [m][N]; columns >= nvalid masked"""
    C = np.asarray(C_rows, np.float64).copy()
    C[:, nvalid:] = -np.inf
    m, N = C.shape
    G = C.reshape(m, N // 64, 64)
    mx = G.max(2)
    with np.errstate(invalid="ignore"):
        sm = np.where(np.isfinite(mx), np.exp(G - np.where(np.isfinite(mx), mx, 0.0)[..., None]).sum(2), 0.0)
    return mx, sm


def rowsum2_ref(C_rows):
    """(sum, sum of squares) * 2^20 of stored rows and the bound of the int64 result"""
    C = np.asarray(C_rows, np.float64)
    N = C.shape[1]
    s = np.stack([C.sum(1), (C * C).sum(1)], 1) * 2.0 ** 20
    b = 2.0 ** 20 * 2 * 128 * U32 * np.stack([np.abs(C).sum(1), (C * C).sum(1)], 1) + N / 32 + 1
    return s, b


def ln_fold_params(stats, width, eps):
    """mu, rstd and the relative error bound of the kernel's fp32 rstd from the int64 (sum, sum of squares) x 2^20 row stats"""
    st = np.asarray(stats, np.float64) * 2.0 ** -20
    mu = st[:, 0] / width
    ex2 = st[:, 1] / width
    var = np.maximum(ex2 - mu * mu, 0.0)
    rstd = 1.0 / np.sqrt(var + eps)
    d_rstd = U32 * (ex2 + mu * mu) / (var + eps) + 4 * U32
    return mu, rstd, d_rstd


def check(got, ref, bound, what="C", *, log=True) -> float:
    """|got - ref| <= bound per element (NaN anywhere fails).  Prints and returns the worst err / bound."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    bound = np.asarray(bound, np.float64)
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    ratio = np.where(np.isnan(got) | np.isnan(ref), np.inf, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    if log:
        print(f"[conformance] {what}: worst err/bound {worst:.3g} over {ratio.size} elements")
    if not worst <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: |got - ref| > bound at {i}: got {got[i]!r} ref {ref[i]!r} bound {bound[i]!r} "
                             f"({int((ratio > 1).sum())} of {ratio.size} elements out of bound)")
    return worst


SENTINEL_BF16 = 0x7FA5       # a NaN payload no kernel computes
SENTINEL_F32 = 0x7FA5A5A5
SENTINEL_I64 = 0x7FA5A5A5A5A5A5A5


def sentinel_fill(t):
    """fill a torch tensor (bf16 / fp32 / int64 / fp8) with the canary bit pattern"""
    import torch

    if t.dtype == torch.bfloat16:
        t.view(torch.int16).fill_(SENTINEL_BF16)
    elif t.dtype == torch.float32:
        t.view(torch.int32).fill_(SENTINEL_F32)
    elif t.dtype == torch.int64:
        t.fill_(SENTINEL_I64)
    else:
        t.view(torch.uint8).fill_(0xA5)
    return t


def check_canary(t, window=None, what="C"):
    """every element of the allocation `t` outside `window` (an index into t: a tuple of slices, default (slice(rows), slice(cols))
    given as (rows, cols) ints) still holds the canary bits"""
    import torch

    iv = {torch.bfloat16: (torch.int16, SENTINEL_BF16), torch.float32: (torch.int32, SENTINEL_F32), torch.int64: (torch.int64, SENTINEL_I64)}
    if t.dtype in iv:
        dt, s = iv[t.dtype]
        bits = t.view(dt).clone()
    else:
        bits, s = t.view(torch.uint8).clone(), 0xA5
    if window is not None:
        if isinstance(window[0], int):
            window = (slice(0, window[0]), slice(0, window[1]))
        bits[window] = s
    n = int((bits != s).sum().item())
    if n:
        idx = (bits != s).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n} element(s) outside the output window changed, first at {idx}")


# ------------------------------------------------------------------------------------------------ fp32 GEMM (parity mode)
# The kernel contract of gemm_f32_kernel + epilogue_store in numpy fp32, on the materialised problems of tests/util_gemm_f32_cases.py,
# and the comparison of one problem with the fp64 reference.  The emulation reads the operand ALLOCATIONS through the kernel's own
# strides and guards (so a wrong stride or guard meets the NaN padding), steps k by 16 in ascending order with one rounding per
# multiply-add, and follows the header's epilogue order with the formulas of csrc/common.h on correctly rounded exp2 / rcp / erf.
F32 = np.float32
_LOG2E, _GELU_K1, _GELU_K2 = F32(1.4426950408889634), F32(1.5957691216057308), F32(0.07135481627261745)
DEFECTS = ("k_tail_dropped", "col_past_k", "row_past_m", "ldz_for_r", "drop_idx_ldc", "alpha_after_bias", "bias_after_act",
           "act_unrounded", "acc_ignored", "dact_wrong_id", "sam_sak_swapped", "gelu_tanh_nan")


def _fma32(a, b, c):
    """fp32 fused multiply-add through fp64: the product of two fp32 numbers is exact there, the sum rounds to 53 bits and then to
    24 (the double rounding moves a result only when the 53-bit sum lies within 2^-29 ulp of an fp32 tie)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64) + np.asarray(c, F32).astype(np.float64)).astype(F32)


def _sigmoid_neg_log2(zl):
    with np.errstate(over="ignore", under="ignore"):
        return (F32(1) / (F32(1) + np.exp2(np.asarray(zl, F32).astype(np.float64)).astype(F32))).astype(F32)


def _erf32(x):
    return _erf(np.asarray(x, F32).astype(np.float64)).astype(F32)


def emu_act_fwd(act, x, defect=None):
    """act_fwd of csrc/common.h in fp32.  defect: 'gelu_tanh_nan' (NaN for x <= -64)"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if act == 1:
            return ((F32(0.5) * x) * (F32(1) + _erf32(x * F32(0.70710678118654752)))).astype(F32)
        if act == 2:
            p = _fma32(-_GELU_K2 * _LOG2E, x * x, -_GELU_K1 * _LOG2E)
            y = (x * _sigmoid_neg_log2(x * p)).astype(F32)
            return np.where(x <= -64, F32(np.nan), y) if defect == "gelu_tanh_nan" else y
        if act == 3:
            return (x * _sigmoid_neg_log2(x * (F32(-1.702) * _LOG2E))).astype(F32)
    return x


def emu_act_bwd(act, x):
    """act_bwd of csrc/common.h in fp32"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == 1:
            cdf = F32(0.5) * (F32(1) + _erf32(x * F32(0.70710678118654752)))
            return (cdf + (x * F32(0.3989422804014327)) * np.exp(((F32(-0.5) * x) * x).astype(np.float64)).astype(F32)).astype(F32)
        if act == 2:
            x2 = x * x
            s = _sigmoid_neg_log2(x * _fma32(-_GELU_K2 * _LOG2E, x2, -_GELU_K1 * _LOG2E))
            return _fma32((x * s) * (F32(1) - s), _fma32(F32(3) * _GELU_K2, x2, _GELU_K1), s)
        if act == 3:
            s = _sigmoid_neg_log2(x * (F32(-1.702) * _LOG2E))
            return _fma32((F32(1.702) * x) * s, F32(1) - s, s)
    return np.ones_like(x)


def canary_alloc(rows, ld):
    return np.full((rows, ld), SENTINEL_F32, np.uint32).view(F32)


def canary_intact(t, M, N) -> bool:
    """every element of the fp32 allocation `t` outside [M][N] still holds the canary bits"""
    bits = np.ascontiguousarray(t).view(np.uint32).copy()
    bits[:M, :N] = SENTINEL_F32
    return bool((bits == SENTINEL_F32).all())


def _read(buf, idx):
    """buf as the kernel sees it, a base pointer: flat[idx]; beyond the allocation reads NaN"""
    flat = buf.reshape(-1)
    ok = (idx >= 0) & (idx < flat.size)
    return np.where(ok, flat[np.where(ok, idx, 0)], F32(np.nan)).astype(F32)


def emu_gemm(h, defect=None):
    """One materialised problem h (util_gemm_f32_cases.materialise) as the kernels compute it, in numpy fp32.  Returns the output
    ALLOCATIONS {'C': [M + 2][ldc], 'Z': [M + 2][ldz] or None}, canary-filled outside what the emulated kernel wrote (bf16 problems:
    Z holds bf16 values in fp32).  defect: one of DEFECTS —
      k_tail_dropped   the K loop stops at K - K % 16            col_past_k       A's guard is gk <= K (B's is right)
      row_past_m       every row guard is gm <= M                ldz_for_r        R read with ldz
      drop_idx_ldc     dropout index m * ldc + n                 alpha_after_bias (acc + bias) * alpha
      bias_after_act   act(acc * alpha) + bias                   act_unrounded    act on v, not on v rounded to the Z dtype
      acc_ignored      C_old not added                           dact_wrong_id    act' of id 2 where 1 is asked
      sam_sak_swapped  a k-major A read with its strides swapped gelu_tanh_nan    GELU-tanh gives NaN for x <= -64
    A row past M read into the tile alone cannot change a valid output (the rows of a GEMM are independent): what shows is the kernel
    that also stores that row, so `row_past_m` moves the guard of the load and of the store together and the canary catches it."""
    from util_rowop_ref import mic_hash

    assert defect is None or defect in DEFECTS, defect
    M, N, K, f = h["M"], h["N"], h["K"], h["f"]
    bf = h["dtype"] == "bf16"
    rz = (lambda v: round_bf16(v).astype(F32)) if bf else (lambda v: v)
    sam, sak = (1, h["lda"]) if h["akm"] else (h["lda"], 1)
    if defect == "sam_sak_swapped" and h["akm"]:
        sam, sak = sak, sam
    sbk, sbn = (h["ldb"], 1) if h["bkm"] else (1, h["ldb"])
    Mr = M + 1 if defect == "row_past_m" else M
    Ka = K + 1 if defect == "col_past_k" else K
    rows, cols = np.arange(Mr, dtype=np.int64), np.arange(N, dtype=np.int64)
    acc = np.zeros((Mr, N), F32)
    for k0 in range(0, K - K % 16 if defect == "k_tail_dropped" else K, 16):
        for k in range(k0, min(k0 + 16, Ka)):
            a = _read(h["A"], rows * sam + k * sak)
            b = _read(h["B"], k * sbk + cols * sbn) if k < K else np.zeros(N, F32)
            acc = _fma32(a[:, None], b[None, :], acc)
    with np.errstate(invalid="ignore", over="ignore"):
        m2, n2 = rows[:, None], cols[None, :]
        alpha = F32(f.get("alpha", 1.0) or 1.0)
        bias = None if h["bias"] is None else h["bias"][:N][None, :]
        if bias is not None and defect == "alpha_after_bias":
            v = ((acc + bias) * alpha).astype(F32)
        else:
            v = (acc * alpha).astype(F32)
            if bias is not None and defect != "bias_after_act":
                v = (v + bias).astype(F32)
        out = {"C": canary_alloc(M + 2, h["ldc"]), "Z": None}
        if f.get("zout"):
            out["Z"] = canary_alloc(M + 2, h["ldz"])
            out["Z"][:Mr, :N] = rz(v)
        if f.get("act"):
            v = emu_act_fwd(f["act"], v if defect == "act_unrounded" else rz(v), defect)
            if bias is not None and defect == "bias_after_act":
                v = (v + bias).astype(F32)
        if f.get("dact"):
            d = 2 if (defect == "dact_wrong_id" and f["dact"] == 1) else f["dact"]
            v = (v * emu_act_bwd(d, _read(h["Zin"], m2 * h["ldz"] + n2))).astype(F32)
        if f.get("drop"):
            p = F32(f["drop"])
            thr = np.uint32(min(float(p * F32(4294967296.0)), 4294967295.0))
            idx = (m2 * (h["ldc"] if defect == "drop_idx_ldc" else N) + n2).astype(np.uint32)
            v = np.where(mic_hash(h["seed"] & 0xFFFFFFFF, idx) >= thr, (v * (F32(1) / (F32(1) - p))).astype(F32), F32(0))
        if h["R"] is not None:
            v = (v + _read(h["R"], m2 * (h["ldz"] if defect == "ldz_for_r" else h["ldr"]) + n2)).astype(F32)
        if h["C_old"] is not None:
            out["C"][:M, :N] = h["C_old"]
            if defect != "acc_ignored":
                v = (v + out["C"][:Mr, :N]).astype(F32)
        out["C"][:Mr, :N] = v
    return out


def same_bits(a, b) -> bool:
    return np.array_equal(np.ascontiguousarray(a, F32).view(np.uint32), np.ascontiguousarray(b, F32).view(np.uint32))


def check_problem(h, A, B, C, Z, label, *, log=True):
    """One problem's outputs — the windows C [M][N] (fp32) and Z [M][N] or None — against the fp64 reference on the operand windows
    A [M][K], B [K][N]; returns {'C': worst err / bound, 'Z': ...}.  With a stored Z the reference applies act to THAT z.
    The sweeps of the fp32 kernel use the bare evaluation terms, forward eps_f (|z| + |act(z)|), backward eps_f (1 + |Zin|)^2 |v|
    with v = acc = 1 (those of the bf16 kernels: the bound ref_epilogue carries); on every sweep no output is NaN or +-inf and the
    forward Zout equals the exact pre-activation, rounded to the Z dtype, bit for bit."""
    M, N, f = h["M"], h["N"], h["f"]
    zd = "bf16" if h["dtype"] == "bf16" else "f32"
    win = lambda t: None if t is None else np.asarray(t[:M, :N], np.float64)  # noqa: E731
    epi = dict(alpha=f.get("alpha", 1.0), bias=None if h["bias"] is None else h["bias"][:N].astype(np.float64), act=f.get("act", 0),
               dact=f.get("dact", 0), zin=win(h["Zin"]), R=win(h["R"]), C_old=win(h["C_old"]), c_dtype="f32", z_dtype=zd,
               z_stored=None if Z is None else np.asarray(Z, np.float64))
    if f.get("drop"):
        epi["keep"], epi["drop_p"] = h["keep"], f["drop"]
    with np.errstate(over="ignore"):  # exp(1.702 * 512) of the fp64 QuickGELU: inf, and the quotient 0
        ref = gemm_ref(A, B, **epi)
    bound = ref["bound_C"]
    worst = {}
    if f.get("sweep"):
        assert np.isfinite(np.asarray(C, np.float64)).all(), f"{label}: NaN or inf on the activation grid"
        if f["sweep"] == "fwd":
            z = round_to(h["grid"] * f.get("alpha", 1.0), zd)
            assert same_bits(Z, z), f"{label}: Zout is not the exact pre-activation"
            if zd == "f32":
                bound = EPS_F * (np.abs(z) + np.abs(ref["C"]))
        elif zd == "f32":
            bound = EPS_F * (1 + np.abs(h["grid"])) ** 2
    if Z is not None:
        worst["Z"] = check(Z, ref["Z"], ref["bound_Z"], f"{label} Zout", log=log)
    worst["C"] = check(C, ref["C"], bound, f"{label} C", log=log)
    return worst
