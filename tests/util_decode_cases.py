"""Case tables and seeded input builders of the decode selection conformance suite (tests/test_decode_conformance_{cpu,gpu}.py): the
smallest shapes at which each kernel of csrc/decode.hip in scope can go wrong.  A helper module, not a conftest.

Logits lie on a 2^-4 grid in [-12, 12] (bf16-representable: both storage types see the same numbers, and two different logits are
0.0625 apart — rule 1 of util_decode_ref holds by construction) or are -inf.  The one exception is the radix row of the warpers in
fp32, which needs all 32 key bits; in bf16 it is that row rounded.  Seeds were chosen so that every case is admissible (rule 2, the
top-p margin, the sampling gap); tests/test_decode_conformance_cpu.py asserts that with zero exceptions."""
from __future__ import annotations

import numpy as np

from util_gemm_ref import round_to

DTYPES = ("bf16", "f32")
TNAME = {"bf16": "unsigned short", "f32": "float"}
NEG = -np.inf
BIASES = (0.0, -1.0e7, -3.5, 2.0)   # none, NEG_BIG (merges distinct log-probs into fp32 ties), two running scores

KERNELS = [f"row_lse_topk_kernel<{t}, {km}>" for t in TNAME.values() for km in (8, 16, 32, 64)] + \
          [f"{k}<{t}>" for k in ("row_topk_tiles_kernel", "sample_rows_kernel", "warp_threshold_kernel") for t in TNAME.values()] + \
          ["greedy_step_kernel", "fill_i32_kernel"]
PATTERNS = ("row_lse_topk_kernel<*>", "row_topk_tiles_kernel<*>", "sample_rows_kernel<*>", "warp_threshold_kernel<*>", "greedy_step_kernel",
            "fill_i32_kernel")


def grid(rng, n, lo=-12.0, hi=12.0):
    return rng.integers(int(lo * 16), int(hi * 16) + 1, size=n) / 16.0


def up8(v):
    return (v + 7) // 8 * 8


# ------------------------------------------------------------------------------------------------ mic_row_lse_topk
LSE_V = (7, 8, 9, 65, 2047, 2048, 2049, 8191, 8192, 8193, 16389)   # the loop takes 4 x 256 chunks of 8 columns = 8192 per trip
LSE_K = (1, 2, 8, 9, 16, 17, 32, 33, 64)                          # both edges of the KMAX = 8 / 16 / 32 / 64 builds
LSE_SEED = {8193: 0}                                                    # V -> seed where the default (V) is not admissible
LSE_EDGE_ROWS = ("eqmax40", "allequal", "fewfinite", "ninf_pass", "ramp")
LSE_EDGE_BIAS = (0.0, 2.0, 0.0, -3.5, 0.0)
LSE_MODES = ("plain", "raw", "eos_max", "eos_in_topk", "eos_last")


def lse_ks(V):
    return sorted({min(k, V) for k in LSE_K})


def lse_lds(V):
    return (up8(V), up8(V) + 24)


def lse_kernel_of(k, dtype):
    return f"row_lse_topk_kernel<{TNAME[dtype]}, {8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64}>"


def lse_grid_rows(V):
    """four rows for the four biases"""
    rng = np.random.default_rng(LSE_SEED.get(V, V))
    return grid(rng, (4, V)), np.array(BIASES)


def lse_edge_rows(V):
    rng = np.random.default_rng(1000 + V)
    x = np.empty((5, V))
    x[0] = np.minimum(grid(rng, V), 11.0)
    x[0, 4:44] = 12.0                                  # 40 equal maxima: chunks 0 .. 5, six threads
    x[1] = 1.5                                         # all equal
    x[2] = NEG                                         # fewer than 8 finite entries: tau = -inf, everything is a candidate; for
    for j, c in enumerate(sorted({1, V // 3, V // 2, V - 2, V - 1})):   # k > 5 the -inf tail comes in index order
        x[2, c] = 3.0 - j / 4
    x[3] = grid(rng, V)
    x[3, :8192 if V > 8192 else V // 2] = NEG          # -inf fills the first 8192-column trip of every thread
    x[4] = np.maximum(12.0 - np.arange(V) / 16.0, -12.0)   # descending ramp: thread 0 owns the top 8
    return x, np.array(LSE_EDGE_BIAS)


def lse_mode(x, mode):
    """(x with the EOS column set for the mode, suppress_eos, eos, raw)"""
    V = x.shape[1]
    x = x.copy()
    if mode == "eos_max":
        x[:, V // 2] = 12.0
        return x, True, V // 2, False
    if mode == "eos_in_topk":
        fin = np.isfinite(x[:, V // 3])
        x[fin, V // 3] = 11.5
        return x, True, V // 3, False
    if mode == "eos_last":
        x[:, V - 1] = 12.0
        return x, True, V - 1, False
    return x, False, 2, mode == "raw"


FORCED_K = (1, 8, 64)
FORCED_ROWS = np.array([0, 3, 70, 5, 1000, 63], np.int32)   # 0, ids below k = 8 / 64, ids above


# ------------------------------------------------------------------------------------------------ mic_row_topk_tiles
TILES_K = (1, 8, 15, 16)


def tiles_ntiles(k):
    return sorted({n for n in (1, k - 1, k, k + 1, 255, 256, 257, 4096) if n >= 1})


def tiles_V(ntiles):
    return 262144 if ntiles == 4096 else ntiles * 64 - 13


TILES_ROWS = ("grid", "grid_negbig", "eqgran", "tied_tau", "eos_tau", "ninf")
TILES_BIAS = (0.0, -1.0e7, -3.5, 2.0, 0.0, 0.0)
TILES_SEED = {(257, 16): 0}                            # (ntiles, k) -> seed where the default is not admissible


def tiles_rows(ntiles, k):
    """(x [R][V], biases, eos): R = 6, 2 at the cap (grid and eos_tau).  eos is the column of the spike of granule k - 1 of
    the eos_tau row: with suppress_eos the k-th largest granule maximum is not eligible, tau has to come from the (k + 1)-th"""
    V = tiles_V(ntiles)
    rng = np.random.default_rng(TILES_SEED.get((ntiles, k), 7 * ntiles + k))
    x = np.empty((6, V))
    x[0], x[1] = grid(rng, V), grid(rng, V)
    g0 = np.arange(ntiles) * 64
    width = np.minimum(64, V - g0)
    x[2] = grid(rng, V, -12, 8)                        # every granule maximum equal
    x[2, g0 + (np.arange(ntiles) * 7) % width] = 9.0
    x[3] = grid(rng, V, -12, 0)                        # granules 0, 1 above tau hold elements equal to tau; k granules tied at tau
    if ntiles >= 3:
        x[3, [5, 64 + 9]] = (5.0, 4.0)
        x[3, [1, 17, 40, 64 + 2, 64 + 30]] = 3.0
        tied = np.arange(2, min(ntiles, 2 + k))
        x[3, g0[tied] + (tied * 11) % width[tied]] = 3.0
        x[3, g0[tied[::2]] + (tied[::2] * 11 + 1) % width[tied[::2]]] = 3.0
    x[4] = grid(rng, V, -12, -2)                       # one spike per granule, descending: EOS is the tau granule's only maximum
    sp = np.arange(min(ntiles, k + 2))
    x[4, g0[sp] + 7] = 10.0 - sp / 2
    eos = int(g0[min(k, ntiles) - 1] + 7)
    x[5] = grid(rng, V)                                # -inf granules
    if ntiles >= 3:
        x[5, 64:128] = NEG
        x[5, g0[-1]:] = NEG
    bias = np.array(TILES_BIAS)
    if ntiles == 4096:
        return x[[0, 4]], bias[[0, 4]], eos
    return x, bias, eos


# ------------------------------------------------------------------------------------------------ mic_warp_thresholds
WARP_V = (1, 5, 1023, 1024, 1025, 2049, 5003)          # 1024 threads, radix 11 + 11 + 10 bits
WARP_P = (1e-4, 0.5, 0.9, 1.0)
WARP_T = (1.0, 0.7, 2.0)
WARP_ROWS = ("grid", "signed_zero", "radix", "ties")
WARP_SEED = {1023: 0, 1025: 1, 2049: 7, 5003: 35}      # V -> seed where the default is not admissible
ZERO_ROW = np.array([0.0, -0.0, -0.0, 0.0, -1.0])      # top_k = 3 keeps indices 0, 1, 2 (lax.top_k: 0 == -0)


def zero_row(V, rng):
    """two +0 in front of many -0: a top-k of 3 and every top-p cut need entries of the -0 bin of keys that tell the zeros apart.
    (V = 5 is not ZERO_ROW itself: its four equal masses put a sorted position on top_p = 0.5 exactly at top_k = 4; the worked
    example has tests of its own)"""
    if V <= 5:
        return np.array([0.0, -0.0, -0.5, -0.0, -1.0])[:V]
    x = np.resize(np.array([-0.0, -0.0, -1.0, -0.0]), V)
    x[5 + rng.choice(V - 5, int(rng.integers(0, V // 8 + 1)), replace=False)] = -2.0   # (moves Z: a seed can clear the top-p margin)
    x[:5] = ZERO_ROW
    return x


def warp_ks(V):
    return sorted({0, 1, min(3, V), max(V - 1, 0), V, V + 5})


def warp_combos(V):
    """(top_k, top_p, temperature, suppress_eos) — every top_k x top_p, temperature and suppression cycling over them"""
    out = []
    for i, k in enumerate(warp_ks(V)):
        for j, p in enumerate(WARP_P):
            out.append((k, p, WARP_T[(i + j) % 3], (i + j) % 2 == 1))
    return out


def warp_rows(V, dtype):
    rng = np.random.default_rng(WARP_SEED.get(V, 31 * V))
    x = np.empty((4, V))
    x[0] = grid(rng, V)                                            # negative and positive values mixed
    x[1] = zero_row(V, rng)                                             # zeros of both signs around the top-k and the top-p cut
    # radix: a third shares the top 11 key bits (sign, exponent, 2 mantissa bits), a third the top 22: each pass decides
    b = np.where(np.arange(V) % 3 == 0, 0x3F800000 | rng.integers(0, 1 << 21, V),
                 np.where(np.arange(V) % 3 == 1, 0x40155400 | rng.integers(0, 1 << 10, V), 0xBF800000 | rng.integers(0, 1 << 21, V)))
    x[2] = round_to(b.astype(np.uint32).view(np.float32).astype(np.float64), dtype)
    x[3] = np.where(np.arange(V) % 2 == 0, 1.0, 0.5)               # many entries equal to the threshold straddling the cut
    x[3, rng.choice(V, min(V, int(rng.integers(1, 3))), replace=False)] = 2.0
    x[3, rng.choice(V, int(rng.integers(0, V // 4 + 1)), replace=False)] = -1.0
    return x


# ------------------------------------------------------------------------------------------------ mic_sample_rows
SAMPLE_V = (1, 7, 1023, 1025, 5003)
SAMPLE_R = (3, 4)                                       # R * V odd (the counter array is padded) and even
SAMPLE_KEY_SEED = {}


def sample_rows_of(R, V):
    """rows: grid, the signed-zero row, grid ... (R of them)"""
    rng = np.random.default_rng(5 * V + R)
    x = grid(rng, (R, V), -6, 6)
    x[1] = zero_row(V, rng)
    return x


SAMPLE_VARIANTS = ("plain", "temperature_eos", "topk1_topk3", "topk_topp")


# ------------------------------------------------------------------------------------------------ mic_greedy_step
GREEDY_B = (1, 63, 64, 65)
GREEDY_LD = (1, 8)
