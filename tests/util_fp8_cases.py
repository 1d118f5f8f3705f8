"""The case tables of the fp8 emission conformance suite (tests/test_fp8_conformance_{cpu,gpu}.py) and their deterministic operands
(numpy only, the same on every machine).  A helper module, not a conftest.  Every shape is the smallest at which the edge it names
is reached."""
from __future__ import annotations

import zlib

import numpy as np

import util_rowop_cases as RC
from util_gemm_ref import round_bf16
from util_fp8_ref import FLT_MAX, FMAX, FMTS  # noqa: F401

F32 = np.float32

# the ten instantiations in scope, as tests/golden/kernel_resources.json names them, and the pattern that selects them there
KERNELS = (["fp8_amax_kernel", "fp8_quantize_kernel", "fp8_roll_kernel", "ln_fwd_kernel<unsigned short, true>"]
           + [f"ln_bwd_kernel<unsigned short, {n}, 8, {m}>" for n in (2, 4) for m in (1, 2)]
           + ["attn_bwd_kernel<unsigned short, true>", "ce_bwd_q8_kernel"])
IN_SCOPE = r"fp8_(amax|quantize|roll)_kernel$|ln_fwd_kernel<unsigned short, true>|ln_bwd_kernel<unsigned short, \d, \d, [12]>|" \
           r"attn_bwd_kernel<unsigned short, true>|ce_bwd_q8_kernel$"


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def bf16(x):
    return round_bf16(x).astype(F32)


def tiny_amax(fmt):
    """just below FMAX / FLT_MAX: FMAX / amax overflows fp32"""
    return float(F32(FMAX[fmt] / FLT_MAX) * F32(0.99))


# ------------------------------------------------------------------------------------------------ quantiser
def all_finite_bf16():
    """256 x 256 fp32 array holding every finite bf16 bit pattern once (65280 of them; the other 256 entries are +0) in a shuffled order"""
    bits = np.arange(65536, dtype=np.uint32)
    bits = bits[(bits & 0x7F80) != 0x7F80]
    assert bits.size == 65280
    allb = np.concatenate([bits, np.zeros(256, np.uint32)])
    _rng("exhaustive").shuffle(allb)
    return (allb << 16).astype(np.uint32).view(F32).reshape(256, 256)


# amax_old of the exhaustive case: None = current scaling (amax pass), 0 (scale 1), a power of two, a non-power of two, a value far
# below the tensor's maximum (most of it saturates), the top of the fp32 range (all but the largest inputs leave as subnormal or
# zero bytes: the tensor's own maximum is the largest finite bf16, nothing lies far above it), and the overflowing scale
EXH_AMAX = {"current": None, "zero": 0.0, "pow2": 2.0 ** -3, "nonpow2": 3.1416, "saturating": 0.37e-3, "top": 3.0e38, "tiny": "tiny"}

# (name, rows, cols, rows_pad, extra ld, extra ldq, extra ldqT): both sides of the 128 x 64 (quantiser) and 64 x 64 (amax) tile edges
GEOMETRY = [
    ("g_3x8", 3, 8, 16, 8, 8, 16),
    ("g_127x72", 127, 72, 128, 16, 8, 16),
    ("g_128x64", 128, 64, 128, 8, 16, 32),
    ("g_129x136", 129, 136, 144, 8, 8, 16),
    ("g_130x1032", 130, 1032, 144, 8, 8, 16),
    ("g_100x64_pad256", 100, 64, 256, 8, 8, 16),     # rows_pad adds a whole pad tile of the quantiser
]
GEOMETRY_BY = {g[0]: g for g in GEOMETRY}
OUT_MODES = ("q", "qT", "both")
GEOMETRY_MAX = -24.0   # the largest magnitude of every geometry source, negative, in its last row and column
BEHIND = 3.0e4   # what the source holds behind `rows` and behind `cols`: larger than every valid element


def geometry_source(name, fmt):
    """the source allocation [rows + 3][ld]: valid region randn * 2 with zeros, +-max placed in the last row / last column, BEHIND elsewhere"""
    _, rows, cols, rows_pad, eld, _, _ = GEOMETRY_BY[name]
    rng = _rng(name, fmt)
    full = np.full((rows + 3, cols + eld), BEHIND, F32)
    v = bf16(rng.standard_normal((rows, cols)) * 2.0)
    v[rng.random((rows, cols)) < 0.05] = 0.0
    v[rows - 1, cols - 1] = GEOMETRY_MAX
    full[:rows, :cols] = v
    return full


# grouped launches: ten items (two tables), mixed formats, shapes and output modes: (rows, cols, rows_pad, fmt, mode, amax_old of the
# delayed run)
GROUPED = [(3, 8, 16, "e4m3", "both", 0.5), (70, 136, 80, "e5m2", "q", 1.5), (128, 64, 128, "e4m3", "qT", 40.0),
           (129, 72, 256, "e5m2", "both", 0.0), (1, 16, 16, "e4m3", "q", 7.0), (65, 64, 80, "e5m2", "qT", 3.0),
           (200, 8, 208, "e4m3", "both", 0.3), (5, 520, 16, "e5m2", "q", 100.0), (64, 64, 64, "e4m3", "both", 9.0),
           (33, 200, 48, "e5m2", "both", 2.0)]


def grouped_source(i):
    rows, cols = GROUPED[i][:2]
    v = bf16(_rng("grouped", i).standard_normal((rows + 2, cols + 8)) * (i + 1))
    v[rows:], v[:, cols:] = BEHIND, BEHIND
    return v


# grouped amax launch: eight items of 64 x 4160 = 65 tiles each, 520 tiles > 512: tiles_per_block = 2, so blocks 32, 97, 162, 227 walk
# the last tile of one item and the first tile of the next.  Even items keep their maximum in their last tile, odd items in their first.
AMAX_WALK = dict(items=8, rows=64, cols=4160)


def amax_walk_source(i):
    rows, cols = AMAX_WALK["rows"], AMAX_WALK["cols"]
    rng = _rng("walk", i)
    v = bf16(rng.standard_normal((rows, cols)))
    c = cols - 1 - int(rng.integers(64)) if i % 2 == 0 else int(rng.integers(64))
    v[int(rng.integers(rows)), c] = -(20.0 + i)
    return v


# the partial table: 1025 quantiser tiles, the maximum in the tile of index 1024
WRAP = dict(rows=131200, cols=64)


def wrap_source():
    rng = _rng("wrap")
    v = bf16(rng.standard_normal((WRAP["rows"], WRAP["cols"])))
    v[131072 + 77, 13] = 12.0
    return v


def roll_inputs():
    """state [5][3] (stride 3), partials [5][1024]: slot 2's table is all zero, slot 4's maximum sits in the last entry"""
    rng = _rng("roll")
    state = rng.random((5, 3)).astype(F32) + F32(1)
    part = np.zeros((5, 1024), F32)
    for s, (n, top) in enumerate([(1, 3.5), (700, 0.25), (0, 0.0), (1024, 9.0), (3, 1e-30)]):
        idx = rng.choice(1024, n, replace=False) if n else []
        part[s, idx] = (rng.random(n) * top).astype(F32)
    part[4, 1023] = 2e-30
    return state, part


# ------------------------------------------------------------------------------------------------ LayerNorm
# widths 8 / 72 / 1024 (two-chunk backward build), 1032 / 2048 (four-chunk); rows that do not fill the forward's last block of 4
LN_SHAPES = [(5, 8), (7, 72), (6, 1024), (5, 1032), (3, 2048)]
LN_WRAP = (1030, 8)   # wave index = row: the maximum in a row >= 1024
LN_DROPOUT = (0.0, 0.1)
LN_SEED = 77


def ln_case(rows, width):
    return dict(name=f"lnq_{rows}x{width}", rows=rows, width=width, kinds="mixed")


def ln_wrap_inputs():
    """1030 x 8: rows of +-1 (|xhat| = 1) and one row, 1027, with a single outlier (|xhat| = sqrt 7)"""
    rows, width = LN_WRAP
    x = np.tile(np.array([1.0, -1.0] * (width // 2)), (rows, 1))
    x[1027] = 0.0
    x[1027, 5] = 4.0
    rng = _rng("lnwrap")
    gamma = (1 + 0.05 * rng.standard_normal(width)).astype(F32).astype(np.float64)
    beta = (0.05 * rng.standard_normal(width)).astype(F32).astype(np.float64)
    return x, gamma, beta


# backward: (rows, width); modes 'dxm' (Q8 = 1) and 'dx' (q8_of_dx, Q8 = 2)
LNB_SHAPES = [(9, 72), (20, 1024), (9, 1032), (5, 2048)]
LNB_MODES = (("dxm", 0.0), ("dxm", 0.1), ("dx", 0.0))   # (mode, dropout of the mask): q8_of_dx emits dx itself, no mask takes part


def lnb_kernel(width, mode):
    return f"ln_bwd_kernel<unsigned short, {2 if width <= 1024 else 4}, 8, {1 if mode == 'dxm' else 2}>"


# ------------------------------------------------------------------------------------------------ attention backward
# B 3, H 2.  layout 'fused3': self-attention, one [rows][3d] byte tensor and one slot; 'kv2': cross, dQ [rows][d] and dK | dV [rows][2d]
def _a(name, Tq, Tk, causal=False, mask=None, layout="fused3", q_len=None, kv_packed=False):
    return dict(name=name, B=3, H=2, Tq=Tq, Tk=Tk, causal=causal, mask=mask, layout=layout, q_len=q_len, kv_packed=kv_packed,
                qscale=1.0, dominant=False, shift=False)


ATTN = [
    _a("aq_self_33_causal", 33, 33, causal=True),
    _a("aq_self_64_causal_masked_tail", 64, 64, causal=True, mask="suffix"),
    _a("aq_cross_64x50", 64, 50, layout="kv2"),
    _a("aq_vit_50x50", 50, 50),
    _a("aq_packed_self", 64, 64, causal=True, q_len=(1, 64, 33), kv_packed=True),
    _a("aq_packed_cross50", 64, 50, layout="kv2", q_len=(64, 1, 9)),
]
ATTN_BY = {c["name"]: c for c in ATTN}
PACK_GAP = 2   # rows between two packed sequences that belong to none


def attn_inputs(c):
    """q, k, v, dout (fp64 of bf16 values), key_mask or None, q_off or None.  Packed: sequences PACK_GAP rows apart"""
    import util_attn_cases as AC

    if c["q_len"] is None:
        q, k, v, do, km = AC.dense_inputs(c, "bf16")
        return q, k, v, do, km, None
    rng = _rng(c["name"])
    HD = c["H"] * 64
    q_off = np.cumsum([0] + [n + PACK_GAP for n in c["q_len"]])[:-1].astype(np.int32)
    total = int(q_off[-1] + c["q_len"][-1] + PACK_GAP)
    nk = total if c["kv_packed"] else c["B"] * c["Tk"]
    q, do = (round_bf16(rng.standard_normal((total, HD))) for _ in range(2))
    k, v = (round_bf16(rng.standard_normal((nk, HD))) for _ in range(2))
    return q, k, v, do, None, q_off


# ------------------------------------------------------------------------------------------------ CE backward
CE_ROWS = (3, 64, 65, 257)              # the edges of the 64-row groups and of the 256-row blocks
CE_V = ((130, 136), (505, 512), (1000, 1024))
CE_LS = (0.0, 0.1)
CE_LOSS_SCALE = 4.0


def ce_inputs(rows, V, Vpad):
    """logits [rows][Vpad] (columns V .. Vpad NaN: read as part of a chunk and discarded), labels (the first below 0, the last beyond V
    when there are at least 3 rows), mask (every third row masked), row_lse (fp64 reference rounded to fp32), denom"""
    import util_rowop_ref as RR

    x, labels, _ = RC.ce_inputs(dict(rows=rows, V=V, mask="ones"), "bf16")
    labels = labels.astype(np.int32)
    labels[0], labels[-1] = -100, V + 3
    mask = (np.arange(rows) % 3 != 2).astype(np.int32)
    lse = RR.ce_rows_ref(x, np.clip(labels, 0, V - 1), 0.0)["lse"].astype(F32).astype(np.float64)
    xp = np.full((rows, Vpad), np.nan)
    xp[:, :V] = x
    return xp, labels, mask, lse, float(mask.sum())
