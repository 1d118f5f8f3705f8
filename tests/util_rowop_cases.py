"""The case table of the row-op conformance suite (tests/test_rowop_conformance_{cpu,gpu}.py) and its deterministic operands.
A helper module, not a conftest.  Every case is the smallest shape at which the branch it names is taken; `claim` names the
kernel instantiation(s) it reaches (kernels_of), which the CPU module checks against the dispatch rules restated here and against
the committed kernel listing of the GPU module."""
from __future__ import annotations

import numpy as np

from util_gemm_ref import round_to

DTYPES = ("bf16", "f32")
T_OF = {"bf16": "unsignedshort", "f32": "float"}
LN_EPS = 1e-5
LNB_WAVES, LNB_CAP = 8, 512


def _c(name, **kw):
    return dict(name=name, **kw)


# ------------------------------------------------------------------------------------------------ LayerNorm
# rows kinds: 'ord' ordinary, 'shift' a large mean, 'tiny' std 1e-3, 'const' a constant row (var = 0: rstd = eps^-1/2); every case
# carries all four (row r has kind r % 4 when mixed)
LN_FWD = [
    _c("ln_1x8", rows=1, width=8, kinds="mixed"),
    _c("ln_3x520", rows=3, width=520, kinds="mixed"),            # a partial forward block; second chunk column holds one chunk
    _c("ln_9x768", rows=9, width=768, kinds="mixed"),
    _c("ln_50x1024", rows=50, width=1024, kinds="mixed"),        # the two-chunk build full
    _c("ln_9x1032", rows=9, width=1032, kinds="mixed"),          # four-chunk build, one chunk in its third column
    _c("ln_3x2048", rows=3, width=2048, kinds="mixed"),
    _c("ln_9x768_shift", rows=9, width=768, kinds="shift"),
    _c("ln_50x64_nostats", rows=50, width=64, kinds="mixed", nostats=True),
]
LN_DROPOUT = (0.0, 0.1)
# the flag combinations engine.py's ln_bwd call sites issue: none (vit.pre_ln), dres (ViT ln1 / ln2, decoder ln_sa of layer 0),
# dxm (dec.ln_f), dres + dxm (ln_ff, ln_ca, ln_sa), in_dropout (dec.ln_emb); 'all' is one more than it issues
LN_FLAGS = {"none": (), "dres": ("dres",), "dxm": ("dxm",), "dres_dxm": ("dres", "dxm"), "in_dropout": ("in_dropout",),
            "all": ("dres", "dxm", "in_dropout")}
LN_BWD = [
    _c("lnb_1x8", rows=1, width=8, flags="dres_dxm"),
    _c("lnb_3x520", rows=3, width=520, flags="none"),
    _c("lnb_9x768", rows=9, width=768, flags="dres"),
    _c("lnb_50x1024", rows=50, width=1024, flags="dxm"),
    _c("lnb_9x1032", rows=9, width=1032, flags="in_dropout"),
    _c("lnb_3x2048", rows=3, width=2048, flags="all"),
    _c("lnb_50x768", rows=50, width=768, flags="dres_dxm"),
    _c("lnb_4107x64", rows=4107, width=64, flags="dres_dxm"),    # the grid-stride trip of the two-chunk build
    _c("lnb_4107x1032", rows=4107, width=1032, flags="dres"),    # ... and of the four-chunk build
    _c("lnb_50x64_nobeta", rows=50, width=64, flags="none", nobeta=True),
]
LN_FOLD = [(5, 8, True), (9, 520, False), (130, 768, True), (4, 1024, True)]   # (N, K, bias)
LN_ALL = {c["name"]: c for c in LN_FWD + LN_BWD}


def ln_bwd_blocks(rows):
    return min(-(-rows // LNB_WAVES), LNB_CAP)


def ln_rows(rows, width, kinds, dtype, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, width)) * 2.0
    for r in range(rows):
        k = ("ord", "shift", "tiny", "const")[r % 4] if kinds == "mixed" else kinds
        if k == "shift":
            x[r] = x[r] / 2.0 + LN_SHIFT
        elif k == "tiny":
            x[r] = 3.0 + 1e-3 * x[r]
        elif k == "const":
            x[r] = 1.5
    return round_to(x, dtype)


LN_SHIFT = 300.0   # chosen on the CPU (test_one_pass_variance_is_caught_by_rstd): emulation < 0.5, one-pass variance > 1


def ln_inputs(c, dtype):
    rows, width = c["rows"], c["width"]
    seed = rows * 7 + width
    rng = np.random.default_rng(seed + 1)
    x = ln_rows(rows, width, c.get("kinds", "mixed" if rows < 100 else "ord"), dtype, seed)
    gamma = (1 + 0.2 * rng.standard_normal(width)).astype(np.float32).astype(np.float64)
    beta = (0.2 * rng.standard_normal(width)).astype(np.float32).astype(np.float64)
    dy = round_to(rng.standard_normal((rows, width)) * 0.5, dtype)
    dres = round_to(rng.standard_normal((rows, width)) * 0.5, dtype)
    return x, gamma, beta, dy, dres


def ln_kernels_of(c, dtype):
    T = T_OF[dtype]
    if "flags" in c:
        return [f"ln_bwd_kernel<{T},{2 if c['width'] <= 1024 else 4},8,0>"]
    return [f"ln_fwd_kernel<{T},false>"]


# ------------------------------------------------------------------------------------------------ cross-entropy
# (rows, V, Vpad, ld); masks: 'ones' | 'one' (all but one zero) | 'alt'
CE = [
    _c("ce_1003", rows=24, V=1003, Vpad=1024, ld=1024, mask="alt"),
    _c("ce_9", rows=5, V=9, Vpad=16, ld=24, mask="ones"),                     # V just above the refusal, ld > Vpad
    _c("ce_8200", rows=70, V=8200, Vpad=8200, ld=8208, mask="one"),           # 1025 chunks: second trip of the U = 4 loop, three chunks absent
    _c("ce_600", rows=300, V=600, Vpad=640, ld=640, mask="alt"),              # the reduce stride loop
    _c("ce_250054", rows=3, V=250054, Vpad=250112, ld=250112, mask="ones", big=True),
    _c("ce_1003_neginf_chunk", rows=24, V=1003, Vpad=1024, ld=1024, mask="alt", neginf=True),
    # at 126 chunks every thread that met a -inf chunk first merges with an absent partner in the LDS tree, whose guard clears the
    # NaN; at 263 chunks thread 0 has a second, finite chunk (NaN * exp(-inf - m)) and a present partner: the NaN reaches row_lse
    _c("ce_2100_neginf_chunk", rows=8, V=2100, Vpad=2104, ld=2112, mask="alt", neginf=True),
]
CE_LS = (0.0, 0.1)
CE_BY = {c["name"]: c for c in CE}


def ce_labels(rows, V):
    """label 0, V - 1, a chunk's first and last lane, then spread"""
    fixed = [0, V - 1, 8 % V, 7 % V, (V - 1) // 8 * 8, min(V - 1, 2047), min(V - 1, 2048)]
    rng = np.random.default_rng(V)
    return np.array([fixed[r] if r < len(fixed) else int(rng.integers(V)) for r in range(rows)], np.int32)


def ce_mask(rows, kind):
    if kind == "ones":
        return np.ones(rows, np.int32)
    if kind == "one":
        m = np.zeros(rows, np.int32)
        m[rows // 2] = 1
        return m
    return (np.arange(rows) % 2 == 0).astype(np.int32)


def ce_inputs(c, dtype):
    """logits [rows][V] as stored, labels, mask.  neginf: rows 1, 5, 9, .. carry -inf in columns [0, 8), rows 2, 6, .. in the whole
    granule [64, 128), row 3 in both; labels lie elsewhere"""
    rows, V = c["rows"], c["V"]
    rng = np.random.default_rng(rows + V)
    x = rng.standard_normal((rows, V)) * 3.0
    x[np.arange(rows), rng.integers(V, size=rows)] += 6.0
    labels, mask = ce_labels(rows, V), ce_mask(rows, c["mask"])
    x = round_to(x, dtype)
    if c.get("neginf"):
        for r in range(rows):
            if r % 4 in (1, 3):
                x[r, 0:8] = -np.inf
            if r % 4 in (2, 3):
                x[r, 64:128] = -np.inf
        labels = np.where((labels < 8) | ((labels >= 64) & (labels < 128)), labels + 200, labels).astype(np.int32)
    return x, labels, mask


def ce_kernels_of(dtype):
    T = T_OF[dtype]
    return [f"ce_rows_kernel<{T}>", f"ce_bwd_kernel<{T}>", "ce_reduce_kernel"]


# ce_rows_tiles: V -> ntiles = ceil(V / 64) = 0, 1, 2, 3 (mod 4), and 258 (a second trip); each with an aligned even stat_ld and with
# an odd stat_ld / a base 8 B into the allocation
CE_TILES = [256, 300, 321, 400, 1003, 1090, 1150, 1200, 16500]   # ntiles 4, 5, 6, 7, 16, 18, 18, 19, 258
TILES_LAYOUT = ("aligned", "odd_ld", "base8")
# ce_bwd_t / transpose: (rows, rows_pad, V, Vpad, ld, ld_t)
CE_T = [
    _c("cet_37", rows=37, rows_pad=0, V=515, Vpad=520, ld=528, ld_t=64),          # one column block, mostly empty
    _c("cet_37_pad128", rows=37, rows_pad=128, V=1003, Vpad=1024, ld=1024, ld_t=136),
    _c("cet_64", rows=64, rows_pad=0, V=1024, Vpad=1024, ld=1024, ld_t=64),
    _c("cet_150", rows=150, rows_pad=0, V=5050, Vpad=5056, ld=5064, ld_t=200),    # Vpad not a multiple of 512, ld_t > rows_pad
]

# ------------------------------------------------------------------------------------------------ AdamW
B1, B2, EPS, WD = 0.9, 0.999, 1e-6, 0.01
ADAMW = [
    _c("adamw_4_t1", n=4, t=1, lr=1e-3),
    _c("adamw_4100_t7", n=4100, t=7, lr=1e-3),
    _c("adamw_4100_t1e5", n=4100, t=100000, lr=1e-3),
    _c("adamw_4100_t1", n=4100, t=1, lr=1e-3),
    _c("adamw_4100_zero", n=4100, t=7, lr=1e-3, zero=True),          # m = v = g = 0: the update is wd * p
    _c("adamw_4100_wd0", n=4100, t=7, lr=1e-3, wd=0.0),
    _c("adamw_4100_lr0", n=4100, t=7, lr=0.0),                       # p keeps its bits, m and v move
    _c("adamw_4100_gs", n=4100, t=7, lr=1e-3, gscale=0.5),
    _c("adamw_4100_nolp", n=4100, t=7, lr=1e-3, nolp=True),
    _c("adamw_8388612", n=8388612, t=7, lr=1e-3, big=True),          # one float4 beyond 8192 x 256: the grid-stride trip
]
ADAMW_BY = {c["name"]: c for c in ADAMW}
ADAMW_ROWS = [(6, 12), (5, 1024), (5, 1028), (3, 2048)]              # 1028 = 257 float4s: a second trip for thread 0 only
ADAMW_FLAGS = ("none", "all", "mixed")


def adamw_inputs(c, n=None):
    n = n or c["n"]
    rng = np.random.default_rng(n % 100003 + int(c["t"]) % 97)
    f = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
    p, m, v, g = f(rng.standard_normal(n)), f(rng.standard_normal(n) * 0.1), f(rng.random(n) * 0.01), f(rng.standard_normal(n))
    if c.get("zero"):
        m, v, g = np.zeros(n), np.zeros(n), np.zeros(n)
    return p, m, v, g


def adamw_hyper(c):
    return dict(lr=c["lr"], t=float(c["t"]), b1=B1, b2=B2, eps=EPS, wd=c.get("wd", WD), gscale=c.get("gscale", 1.0))


# every kernel instantiation in scope and the test of the GPU module that reaches it
KERNELS = (
    [f"ln_fwd_kernel<{T},false>" for T in T_OF.values()]
    + [f"ln_bwd_kernel<{T},{n},8,0>" for T in T_OF.values() for n in (2, 4)]
    + ["ln_param_grads_kernel"]
    + [f"{k}<{T}>" for k in ("ln_fold_weight_kernel", "ce_rows_kernel", "ce_rows_tiles_kernel", "ce_bwd_kernel") for T in T_OF.values()]
    + ["ce_reduce_kernel", "tile_transpose_kernel<0>", "tile_transpose_kernel<1>", "adamw_kernel<false>", "adamw_kernel<true>"]
)
