"""The case table of the fp32 GEMM conformance suite: gemm_f32_kernel (csrc/gemm.hip, the parity mode) with the scalar epilogue
epilogue_store<float> (csrc/common.h), and the activation functions act_fwd / act_bwd at fp32 resolution.  Shared by
tests/test_gemm_f32_conformance_gpu.py (runs every case on the device) and tests/test_gemm_f32_conformance_cpu.py (runs every case
through the numpy fp32 emulation of tests/util_gemm_ref.py: the bounds are reachable, the checker rejects the listed defects).

Conventions of every fp32 case (`materialise` below builds the host data that keeps them):
  - operands sit inside larger allocations: lda / ldb = the contiguous extent + 3 (odd on purpose), 2 extra rows follow;
  - everything outside the [M][K] / [N][K] windows is NaN: one element read beyond the window poisons the result (NaN * 0 = NaN);
    the bias vector is followed by NaN too;
  - three different leading dimensions: ldc = N + 5, ldz = N + 1 (Zout and Zin, as the header says), ldr = N + 9;
  - C, Zout, Zin and R start one element past a 16-byte boundary; C and Zout lie in canary-filled allocations, Zin and R in NaN;
  - inputs are normal numbers or exact zeros (one element in 16 is an exact zero).
The bf16 sweeps go through the bf16 kernels' VECTOR epilogue, which needs what the conventions deny: there lda = ldb = K + 8,
ldc = N + 8, ldz = N + 16, every base 16-B aligned.

Families:
  layouts    the bare epilogue, the four (a_kmajor, b_kmajor) pairs at LAYOUT_SHAPES: one K step and fewer, K % 16 in {0, 1, 15},
             the 32-row wave boundary, the 64-row tile boundary one under and one over;
  epilogue   at EPILOGUE_SHAPES every feature alone, the forward chain and the backward chain (N = 67: m * N + n != m * ldc + n);
  grouped    mic_gemm_grouped with 11 fp32 problems of mixed shapes, layouts and epilogues (the f32 path runs them in sequence;
             the bf16 path launches 8 at a time);
  sweep_*    the activation domain sweep: z = +-mantissa * 2^e, e = -24 .. +8, plus a row of +0 — every product exact, so the
             epilogue sees z itself.  f32: 256 seeded 24-bit mantissas in [1, 2), K = 1, forward (act with Zout) and backward
             (acc = 1, Zin = the grid).  bf16 kernels with an fp32 C: 128 8-bit mantissas, N = 40 (33 columns carry the exponents, 7
             are zero), K = 64 with only k = 0 non-zero, Zout / Zin bf16.  On that grid every pre-activation is a bf16 number, so an
             epilogue that hands act the UNROUNDED value cannot show: the sweep_bf16_fwd_*_alpha cases rerun the forward sweep with
             alpha = 1 + 2^-9 (v needs 17 significant bits; exact in fp32, rounded by the bf16 Zout).

Measured on an MI355X (worst err / bound of a family, from the run of tests/test_gemm_f32_conformance_gpu.py that goes with this
table; the assertion is err <= bound, these figures are what a later reader compares against):
    family                  C        Zout     (the numpy fp32 emulation of tests/util_gemm_ref.py on the same cases)
    layouts                 0.25     -        (0.25)
    epilogue                0.591    0.0417   (0.591, 0.0417)
    grouped                 0.461    0.0747   (0.461, 0.0747)
    sweep_f32_fwd_act1      0.0274   0        (0.0254)        GELU-erf
    sweep_f32_fwd_act2      0.0333   0        (0.0333)        GELU-tanh
    sweep_f32_fwd_act3      0.033    0        (0.031)         QuickGELU
    sweep_f32_bwd_act1      0.0312   -        (0.0312)
    sweep_f32_bwd_act2      0.0388   -        (0.0394)
    sweep_f32_bwd_act3      0.0409   -        (0.0347)
    sweep_bf16_fwd_act1     0.0248   0.498    (0.0248, 0.498; Zout 0 without alpha, 0.498 = the bf16 rounding of the 17-bit v)
    sweep_bf16_fwd_act2     0.0304   0.498    (0.027)
    sweep_bf16_fwd_act3     0.0312   0.498    (0.028)
    sweep_bf16_bwd_act1     0.0102   -        (0.0102)
    sweep_bf16_bwd_act2     0.0249   -        (0.0249)
    sweep_bf16_bwd_act3     0.0139   -        (0.0123)
  The hardware's approximate exp2 / rcp / __expf stay within 0.041 of the eps_f bound over 2^-24 <= |z| < 512: no finding.
  fma-chain report: 0 of 268072 outputs of the layout cases differ from the numpy fp32 chain (k ascending, one rounding per
  multiply-add) — v_mfma_f32_32x32x2_f32 behaves as the fused chain the kernel's header claims, on these inputs.
  Every case passed on the first run; the kernels needed no change.  Two deliberately wrong builds (A's k guard admitting k = K with
  the dropout index taken with ldc; R read with ldz with alpha applied after the bias) failed 59 and 7 of the module's 116 tests.
"""
from __future__ import annotations

import numpy as np

LAYOUT_SHAPES = [(1, 1, 1), (1, 1, 16), (70, 130, 1), (31, 33, 15), (32, 32, 17), (63, 65, 16), (64, 64, 64), (65, 63, 33),
                 (129, 127, 200), (200, 136, 192)]
LAYOUTS = [("nn", False, False), ("nt", False, True), ("tn", True, False), ("tt", True, True)]  # (a_kmajor, b_kmajor)
EPILOGUE_SHAPES = [(96, 72, 48), (65, 67, 40)]
WINDOW_CASE = (129, 127, 200)  # position independence: the sub-problem on rows [64, 129) x columns [64, 127)
WINDOW_AT = (64, 64)
ALPHA_17BIT = 1.0 + 2.0 ** -9
SWEEP_EXPONENTS = list(range(-24, 9))


def prob(M, N, K, *, akm=False, bkm=False, dtype="f32", **feats):
    """one GEMM problem.  feats: alpha, bias, act, zout, dact, drop (p), res, acc, sweep ('fwd' | 'bwd')"""
    return dict(M=M, N=N, K=K, akm=akm, bkm=bkm, dtype=dtype, f=feats)


def case(name, family, *probs, grouped=False):
    return dict(name=name, family=family, probs=list(probs), grouped=grouped)


FEATURES = [("alpha0375", dict(alpha=0.375)), ("alpha_m15", dict(alpha=-1.5)), ("alpha0", dict(alpha=0.0)), ("bias", dict(bias=1)),
            ("act1", dict(act=1)), ("act2", dict(act=2)), ("act3", dict(act=3)),
            ("act1_zout", dict(act=1, zout=1)), ("act2_zout", dict(act=2, zout=1)), ("act3_zout", dict(act=3, zout=1)),
            ("dact1", dict(dact=1)), ("dact2", dict(dact=2)), ("dact3", dict(dact=3)),
            ("drop01", dict(drop=0.1)), ("drop05", dict(drop=0.5)), ("res", dict(res=1)), ("acc", dict(acc=1)),
            ("fwd_chain", dict(alpha=0.375, bias=1, act=2, zout=1, drop=0.1, res=1, acc=1)),
            ("bwd_chain", dict(alpha=-1.5, dact=1, drop=0.5, res=1, acc=1))]

CASES = []
for _M, _N, _K in LAYOUT_SHAPES:
    for _tag, _akm, _bkm in LAYOUTS:
        CASES.append(case(f"layout_{_M}x{_N}x{_K}_{_tag}", "layouts", prob(_M, _N, _K, akm=_akm, bkm=_bkm)))
for _M, _N, _K in EPILOGUE_SHAPES:
    for _tag, _f in FEATURES:
        CASES.append(case(f"epi_{_M}x{_N}x{_K}_{_tag}", "epilogue", prob(_M, _N, _K, **_f)))
CASES.append(case("grouped_eleven_f32", "grouped", *[
    prob(33 + 17 * (i % 4), 20 + 13 * (i % 5), (1, 15, 16, 17, 40, 64, 100)[i % 7], akm=bool(i & 1), bkm=bool(i & 2), **FEATURES[(5 * i + 3) % len(FEATURES)][1])
    for i in range(11)], grouped=True))
for _a in (1, 2, 3):
    CASES.append(case(f"sweep_f32_fwd_act{_a}", f"sweep_f32_fwd_act{_a}", prob(513, 33, 1, sweep="fwd", act=_a, zout=1)))
    CASES.append(case(f"sweep_f32_bwd_act{_a}", f"sweep_f32_bwd_act{_a}", prob(513, 33, 1, sweep="bwd", dact=_a)))
    CASES.append(case(f"sweep_bf16_fwd_act{_a}", f"sweep_bf16_fwd_act{_a}", prob(257, 40, 64, dtype="bf16", sweep="fwd", act=_a, zout=1)))
    CASES.append(case(f"sweep_bf16_bwd_act{_a}", f"sweep_bf16_bwd_act{_a}", prob(257, 40, 64, dtype="bf16", sweep="bwd", dact=_a)))
    CASES.append(case(f"sweep_bf16_fwd_act{_a}_alpha", f"sweep_bf16_fwd_act{_a}",
                      prob(257, 40, 64, dtype="bf16", sweep="fwd", act=_a, zout=1, alpha=ALPHA_17BIT)))

BY_NAME = {c["name"]: c for c in CASES}
FAMILIES = sorted({c["family"] for c in CASES})


def seed_of(name: str, i: int = 0) -> int:
    return 20261021 + 131 * sum(map(ord, name)) + i


def sweep_grid(bits: int, count: int, seed: int):
    """(column [2 count + 1] of +-mantissas with `bits` significant bits in [1, 2) and a final +0, row [33] of 2^e)"""
    rng = np.random.default_rng(seed)
    m = 1.0 + rng.integers(0, 2 ** (bits - 1), size=count).astype(np.float64) * 2.0 ** -(bits - 1)
    m[0], m[1] = 1.0, 2.0 - 2.0 ** -(bits - 1)  # both ends of the binade
    return np.concatenate([m, -m, [0.0]]), 2.0 ** np.array(SWEEP_EXPONENTS, np.float64)


def _padded(rows, cols, ld, pad_rows, win):
    t = np.full((rows + pad_rows, ld), np.nan, np.float32)
    t[:rows, :cols] = win
    return t


def _randn(rng, shape, scale=1.0):
    """fp32 normal numbers with one exact zero in 16"""
    x = (rng.standard_normal(shape) * scale).astype(np.float32)
    return np.where(rng.random(shape) < 1 / 16, np.float32(0), x)


def materialise(p, seed):
    """the host data of one problem under the conventions above: a dict of numpy fp32 arrays (bf16 problems: bf16 values held in fp32).
    A / B / Zin / R / bias: whole allocations (NaN outside the windows); C_old [M][N]; keep [M][N] bool; the leading dimensions and
    `off`, the element offset of C / Zout / Zin / R past a 16-byte boundary."""
    from util_rowop_ref import keep_mask

    M, N, K, f = p["M"], p["N"], p["K"], p["f"]
    bf = p["dtype"] == "bf16"
    rng = np.random.default_rng(seed)
    opad = 8 if bf else 3
    h = dict(M=M, N=N, K=K, akm=p["akm"], bkm=p["bkm"], dtype=p["dtype"], f=f, off=0 if bf else 1, seed=seed,
             ldc=N + (8 if bf else 5), ldz=N + (16 if bf else 1), ldr=N + (8 if bf else 9))
    Aw, Bw = _randn(rng, (M, K)), _randn(rng, (K, N))
    zin = _randn(rng, (M, N), 1.5) if f.get("dact") else None
    if f.get("sweep"):
        col, row = sweep_grid(8 if bf else 24, 128 if bf else 256, seed)
        grid = np.zeros((M, N))
        grid[:, :len(row)] = np.outer(col, row)
        Aw, Bw = np.zeros((M, K), np.float32), np.zeros((K, N), np.float32)
        if f["sweep"] == "fwd":
            Aw[:, 0], Bw[0, :len(row)] = col, row
        else:
            Aw[:, 0], Bw[0, :], zin = 1.0, 1.0, grid.astype(np.float32)
        h["grid"] = grid
    h["A"] = _padded(K, M, M + opad, 2, Aw.T) if p["akm"] else _padded(M, K, K + opad, 2, Aw)
    h["B"] = _padded(K, N, N + opad, 2, Bw) if p["bkm"] else _padded(N, K, K + opad, 2, Bw.T)
    h["lda"], h["ldb"] = h["A"].shape[1], h["B"].shape[1]
    h["bias"] = np.concatenate([_randn(rng, (N,)), np.full(4, np.nan, np.float32)]) if f.get("bias") else None
    h["Zin"] = _padded(M, N, h["ldz"], 2, zin) if zin is not None else None
    h["R"] = _padded(M, N, h["ldr"], 2, _randn(rng, (M, N), 4.0)) if f.get("res") else None
    h["C_old"] = _randn(rng, (M, N), 8.0) if f.get("acc") else None
    h["keep"] = keep_mask(M * N, f["drop"], seed & 0xFFFFFFFF).reshape(M, N) if f.get("drop") else None
    return h


def windows(h):
    """(A [M][K], B [K][N]) of a materialised problem, fp64"""
    M, N, K = h["M"], h["N"], h["K"]
    A = h["A"][:K, :M].T if h["akm"] else h["A"][:M, :K]
    B = h["B"][:K, :N] if h["bkm"] else h["B"][:N, :K].T
    return A.astype(np.float64), B.astype(np.float64)
