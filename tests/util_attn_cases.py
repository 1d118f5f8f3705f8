"""The case table of the attention conformance suite, shared by tests/test_attn_conformance_gpu.py (which runs every case in
both storage types) and tests/test_attn_conformance_cpu.py (which asserts that each case still reaches the kernel it claims, by a
pure mirror of the dispatch rules of csrc/attention.hip, and that the committed kernel trace holds every claimed instantiation).

`claim` names the kernel family the case was written for:
    dense / packed / probs:  'single' (attn_fwd_kernel, attn_bwd_kernel<T, false>), 'tiled' (attn_fwd_tiled_kernel,
                             attn_bwd_tiled_kernel<T, 0 / 1>), 'probs'
    decode:                  'group2' / 'group4' / 'group8', 'row' (attn_decode_kernel<T, false>), 'chunked' (<T, true>)
Masks (key_mask_of): 'suffix' (right padding, the product's), 'holes' (masked keys in the middle), 'key0' (key 0 masked, no
causal), 'first_block' (keys 0..63 of one batch entry masked), 'middle_block' (keys 64..127), 'nokey' (with causal: key 0 of batch
entry 1 masked, so its query 0 has no admissible key; batch entry 2 entirely masked)."""
import numpy as np

T_NAME = {"bf16": "unsigned short", "f32": "float"}
DTYPES = ("bf16", "f32")


def _d(name, B, H, Tq, Tk, claim, causal=False, mask=None, layout="sep", qscale=1.0, dominant=False, shift=False):
    return dict(name=name, B=B, H=H, Tq=Tq, Tk=Tk, claim=claim, causal=causal, mask=mask, layout=layout, qscale=qscale,
                dominant=dominant, shift=shift)


DENSE = [
    # the product's three shapes (layouts as the engine's: fused [rows][3d] q|k|v, cross k|v in one [rows][2d] buffer)
    _d("vit_50x50", 3, 12, 50, 50, "single", layout="fused3"),
    _d("dec_64x64_b64", 64, 16, 64, 64, "single", causal=True, mask="suffix", layout="fused3"),  # 1024 workgroups
    _d("cross_64x50", 3, 16, 64, 50, "single", layout="kv2"),
    # one tile, ragged
    _d("t_1x1", 2, 2, 1, 1, "single"),
    _d("t_1x64", 2, 3, 1, 64, "single", layout="kv2"),
    _d("t_64x1", 2, 3, 64, 1, "single"),
    _d("t_31x33", 3, 3, 31, 33, "single", mask="suffix"),
    _d("t_32x32_causal", 2, 3, 32, 32, "single", causal=True, layout="fused3"),
    _d("t_33x31_causal", 3, 2, 33, 31, "single", causal=True, mask="suffix"),
    _d("t_31x64_causal", 2, 3, 31, 64, "single", causal=True, layout="kv2"),
    _d("t_64x32_causal", 2, 3, 64, 32, "single", causal=True),
    _d("t_63x64_holes", 3, 3, 63, 64, "single", mask="holes", layout="kv2"),
    _d("t_64x63_causal_holes", 3, 2, 64, 63, "single", causal=True, mask="holes"),
    _d("t_63x33_key0", 3, 3, 63, 33, "single", mask="key0"),
    _d("t_64x64_x4", 2, 3, 64, 64, "single", causal=True, qscale=4.0, dominant=True, layout="fused3"),
    _d("t_50x50_shift", 2, 3, 50, 50, "single", shift=True, layout="fused3"),
    # more than one tile
    _d("m_65x65_causal", 2, 2, 65, 65, "tiled", causal=True, layout="fused3"),
    _d("m_127x127", 2, 3, 127, 127, "tiled", mask="holes", layout="fused3"),
    _d("m_128x128_causal", 3, 4, 128, 128, "tiled", causal=True, mask="suffix", layout="fused3"),
    _d("m_129x129_causal", 2, 2, 129, 129, "tiled", causal=True),
    _d("m_197x197", 3, 3, 197, 197, "tiled", layout="fused3"),
    _d("m_200x200_causal_holes", 3, 2, 200, 200, "tiled", causal=True, mask="holes", layout="fused3"),
    _d("m_50x197", 2, 3, 50, 197, "tiled", layout="kv2"),
    _d("m_50x197_causal", 2, 3, 50, 197, "tiled", causal=True, layout="kv2"),
    _d("m_130x50", 2, 3, 130, 50, "tiled", layout="kv2"),
    _d("m_130x50_causal", 2, 3, 130, 50, "tiled", causal=True, mask="suffix"),
    _d("m_64x128_first_block_masked", 3, 2, 64, 128, "tiled", mask="first_block", layout="kv2"),
    _d("m_200x200_causal_middle_block_masked", 3, 2, 200, 200, "tiled", causal=True, mask="middle_block"),
    _d("m_129x197_x4_dominant", 2, 3, 129, 197, "tiled", qscale=4.0, dominant=True),
    _d("m_65x200_x8_dominant", 2, 2, 65, 200, "tiled", qscale=8.0, dominant=True, layout="kv2"),
    _d("m_128x130_shift", 2, 2, 128, 130, "tiled", shift=True),
    # a row with no admissible key: out row 0, lse -inf, no gradient from it (include/mic_hip.h)
    _d("t_64x64_causal_nokey", 3, 3, 64, 64, "single", causal=True, mask="nokey", layout="fused3"),
    _d("t_33x50_nokey", 3, 2, 33, 50, "single", mask="nokey", layout="kv2"),
    _d("m_130x130_causal_nokey", 3, 2, 130, 130, "tiled", causal=True, mask="nokey", layout="fused3"),
    _d("m_64x197_nokey", 3, 2, 64, 197, "tiled", mask="nokey", layout="kv2"),
]


def _p(name, H, Tq_max, Tk, q_len, kv_packed, causal, layout, dense_twin=False):
    return dict(name=name, B=len(q_len), H=H, Tq_max=Tq_max, Tk=Tk, q_len=list(q_len), kv_packed=kv_packed, causal=causal, layout=layout,
                dense_twin=dense_twin, claim="single")


PACKED = [
    _p("p_self_mixed", 16, 64, 64, (1, 9, 33, 40, 64, 17, 64), 1, True, "fused3"),
    _p("p_self_tqmax48", 3, 48, 48, (1, 9, 33, 40, 48), 1, True, "fused3"),
    _p("p_cross50_mixed", 16, 64, 50, (64, 1, 9, 33, 40, 64), 0, False, "kv2"),
    _p("p_cross64_mixed", 3, 64, 64, (40, 64, 1, 9, 33), 0, False, "kv2"),
    _p("p_self_all64", 3, 64, 64, (64, 64, 64, 64), 1, True, "fused3", dense_twin=True),
    _p("p_cross50_all64", 3, 64, 50, (64, 64, 64), 0, False, "kv2", dense_twin=True),
]

PROBS = [
    dict(name="pr_vit_50x50", B=2, H=12, Tq=50, Tk=50, causal=False, mask=None, claim="probs"),
    dict(name="pr_dec_64x64", B=3, H=16, Tq=64, Tk=64, causal=True, mask="suffix", claim="probs"),
    dict(name="pr_cross_64x50", B=2, H=16, Tq=64, Tk=50, causal=False, mask=None, claim="probs"),
    dict(name="pr_65x65_causal", B=3, H=2, Tq=65, Tk=65, causal=True, mask="holes", claim="probs"),
    dict(name="pr_9x1024", B=3, H=2, Tq=9, Tk=1024, causal=False, mask="holes", claim="probs"),
    dict(name="pr_130x1024_causal", B=2, H=1, Tq=130, Tk=1024, causal=True, mask="suffix", claim="probs"),
    dict(name="pr_33x50_nokey", B=3, H=2, Tq=33, Tk=50, causal=True, mask="nokey", claim="probs"),
]


def _dec(name, R, H, max_len, cur, claim, src=False, row_div=1, ldc2=False, dominant=False):
    return dict(name=name, R=R, H=H, max_len=max_len, cur=cur, claim=claim, src=src, row_div=row_div, ldc2=ldc2, dominant=dominant)


DECODE = [
    _dec("d_div1", 6, 3, 50, 49, "row"),
    _dec("d_group2", 12, 3, 50, 49, "group2", row_div=2, ldc2=True),
    _dec("d_group4", 16, 16, 50, 49, "group4", row_div=4, ldc2=True),
    _dec("d_group8", 16, 3, 64, 63, "group8", row_div=8),
    _dec("d_group4_1slot", 8, 2, 16, 0, "group4", row_div=4),
    _dec("d_group2_clamped", 8, 2, 33, 40, "group2", row_div=2),           # cur + 1 > max_len: every slot of the cache
    _dec("d_div3", 6, 3, 50, 49, "row", row_div=3, ldc2=True),
    _dec("d_div4_ragged_rows", 6, 3, 50, 49, "row", row_div=4),           # R % row_div != 0
    _dec("d_div4_65slots", 8, 2, 65, 64, "chunked", row_div=4, ldc2=True),
    _dec("d_div4_200slots", 8, 2, 200, 199, "chunked", row_div=4),
    _dec("d_src_1", 6, 3, 64, 0, "row", src=True),
    _dec("d_src_8", 6, 3, 64, 7, "row", src=True),
    _dec("d_src_63", 6, 16, 64, 62, "row", src=True),
    _dec("d_src_64", 6, 3, 64, 63, "row", src=True, dominant=True),
    _dec("d_src_64_of_200", 6, 3, 200, 63, "row", src=True),
    _dec("d_src_65", 6, 3, 200, 64, "chunked", src=True, dominant=True),
    _dec("d_src_128", 6, 3, 130, 127, "chunked", src=True, ldc2=True),
    _dec("d_src_200", 6, 3, 200, 199, "chunked", src=True, dominant=True),
    _dec("d_src_clamped_200", 5, 2, 200, 230, "chunked", src=True),
    _dec("d_src_clamped_64", 5, 2, 64, 70, "row", src=True),
]

# (R, HD, max_len, cur): slot 0, a middle slot, the last slot; the sources are the halves of one [R][2 HD + pad] buffer (ldk != HD)
KV_APPEND = [(6, 192, 16, 0), (6, 192, 16, 5), (6, 192, 16, 15), (3, 1024, 200, 199)]

ALL = DENSE + PACKED + PROBS + DECODE
BY_NAME = {c["name"]: c for c in ALL}
assert len(BY_NAME) == len(ALL)


def key_mask_of(c):
    """int32 [B][Tk] (1 = attend) or None"""
    kind = c.get("mask")
    if kind is None:
        return None
    B, Tk = c["B"], c["Tk"]
    km = np.ones((B, Tk), np.int32)
    if kind == "suffix":
        km[1 % B, max(Tk - 3, 1):] = 0
        km[2 % B, max(Tk // 2, 1):] = 0
    elif kind == "holes":
        km[0, 1::3] = 0
        km[1 % B, Tk // 3: Tk // 2] = 0
        km[B - 1, [Tk // 2, Tk - 1]] = 0
    elif kind == "key0":
        km[1:, 0] = 0
        km[B - 1, Tk // 2] = 0
    elif kind == "first_block":
        km[1, :64] = 0
    elif kind == "middle_block":
        km[1, 64:128] = 0
    elif kind == "nokey":
        km[1, 0] = 0
        km[2, :] = 0
    else:
        raise ValueError(kind)
    return km


# ---- the dispatch rules of csrc/attention.hip, restated
def dense_dispatch(Tq, Tk):
    return "tiled" if (Tq > 64 or Tk > 64) else "single"


def decode_dispatch(R, max_len, cur, has_src_row, row_div):
    chunked = min(cur + 1, max_len) > 64
    if not has_src_row and not chunked and row_div in (2, 4, 8) and R % row_div == 0:
        return f"group{row_div}"
    return "chunked" if chunked else "row"


def dispatch_of(c):
    if c["claim"] == "probs":
        return "probs"
    if "R" in c:
        return decode_dispatch(c["R"], c["max_len"], c["cur"], c["src"], c["row_div"])
    if "q_len" in c:
        return dense_dispatch(c["Tq_max"], c["Tk"])
    return dense_dispatch(c["Tq"], c["Tk"])


def kernels_of(claim, dtype):
    """the instantiations (as a kernel trace names them) a case with this claim launches in storage type `dtype`"""
    T = T_NAME[dtype]
    return {"single": [f"attn_fwd_kernel<{T}>", f"attn_bwd_kernel<{T}, false>"],
            "tiled": [f"attn_fwd_tiled_kernel<{T}>", f"attn_bwd_tiled_kernel<{T}, 0>", f"attn_bwd_tiled_kernel<{T}, 1>"],
            "probs": [f"attn_probs_kernel<{T}>"],
            "group2": [f"attn_decode_group_kernel<{T}, 2>"], "group4": [f"attn_decode_group_kernel<{T}, 4>"],
            "group8": [f"attn_decode_group_kernel<{T}, 8>"],
            "row": [f"attn_decode_kernel<{T}, false>"], "chunked": [f"attn_decode_kernel<{T}, true>"],
            "kv_append": [f"kv_append_kernel<{T}>"]}[claim]


# ---- the cases' operands: fp64 arrays of values exact in the storage type, the same on every machine (numpy generator)
def _rng(c, dtype):
    import zlib

    return np.random.default_rng(zlib.crc32(f"{c['name']}/{dtype}".encode()))


def _round(x, dtype):
    import util_gemm_ref as GR

    return GR.round_to(x, dtype)


def dense_inputs(c, dtype):
    """q [B*Tq][H*64], k, v [B*Tk][H*64], dout [B*Tq][H*64], key_mask [B][Tk] or None"""
    rng = _rng(c, dtype)
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    q = rng.standard_normal((B * Tq, H * 64)) * c["qscale"]
    k, v = rng.standard_normal((B * Tk, H * 64)), rng.standard_normal((B * Tk, H * 64))
    do = rng.standard_normal((B * Tq, H * 64))
    if c["dominant"]:  # a key of the last block whose score leads for half of the queries
        k.reshape(B, Tk, H * 64)[:, Tk - 2] *= 3.0
    if c["shift"]:     # 16 * 10 / 8 = 20 added to every score
        q[:, 0::64], k[:, 0::64] = 16.0, 10.0
    return tuple(_round(t, dtype) for t in (q, k, v, do)) + (key_mask_of(c),)


def packed_inputs(c, dtype):
    """q (and, kv_packed, k and v) [sum q_len][H*64]; else k, v [B*Tk][H*64]; dout [sum q_len][H*64]; q_off int32 [B]"""
    rng = _rng(c, dtype)
    H, total = c["H"], sum(c["q_len"])
    nk = total if c["kv_packed"] else c["B"] * c["Tk"]
    q, do = rng.standard_normal((total, H * 64)), rng.standard_normal((total, H * 64))
    k, v = rng.standard_normal((nk, H * 64)), rng.standard_normal((nk, H * 64))
    q_off = np.concatenate([[0], np.cumsum(c["q_len"])[:-1]]).astype(np.int32)
    return tuple(_round(t, dtype) for t in (q, k, v, do)) + (q_off,)


def decode_inputs(c, dtype):
    """q [R][H*64]; kc, vc [rows + 1][max_len][H*64] with NaN in every slot >= n = min(cur + 1, max_len), in cache row 1 when a
    src_row table can avoid it, and in the last row (named only by the src_row entries of slots >= n, which are never read);
    src_row int32 [R][max_len] or None"""
    rng = _rng(c, dtype)
    R, H, L = c["R"], c["H"], c["max_len"]
    n = min(c["cur"] + 1, L)
    rows = R if c["src"] else -(-R // c["row_div"])
    q = _round(rng.standard_normal((R, H * 64)), dtype)
    kc, vc = (_round(rng.standard_normal((rows + 1, L, H * 64)), dtype) for _ in range(2))
    if c["dominant"]:
        kc[:, max(n - 2, 0)] = _round(kc[:, max(n - 2, 0)] * 5.0, dtype)
    src = None
    if c["src"]:
        named = np.array([r for r in range(rows) if r != 1])
        src = named[rng.integers(0, len(named), (R, L))].astype(np.int32)
        src[:, n:] = rows
        kc[1], vc[1] = np.nan, np.nan
    kc[:, n:], vc[:, n:] = np.nan, np.nan
    kc[rows], vc[rows] = np.nan, np.nan
    return q, kc, vc, src
