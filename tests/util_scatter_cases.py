"""Case tables of the gather / scatter conformance suite (tests/test_scatter_conformance_{cpu,gpu}.py): the embeddings, the ViT
assembly, the column sums and the small data-movement kernels of csrc/elementwise.hip.  A helper module, not a conftest.

Every case is the smallest shape that takes one branch of its kernel or of its host dispatch; the comment beside it names the
branch.  The dispatch rules of the host code are restated here (`*_kernels_of`, `colsum_plan`, `cast_split`, ...) so that the CPU
module can check each case's claim and the coverage of the build.  Operands are float64 arrays of values exact in their storage
type, produced from a seed: the CPU and the GPU module see the same numbers."""
from __future__ import annotations

import re

import numpy as np

from util_gemm_ref import round_to

DTYPES = ("bf16", "f32")
TN = {"bf16": "unsigned short", "f32": "float"}
# the instantiations in scope, by name: anything a later build adds under these names needs a case
IN_SCOPE = re.compile(r"^(im2col8?_kernel|vit_assemble(_bwd8?)?_kernel|embed_(fwd|bwd)_kernel|det_(owner|single|multi|reset)_kernel|"
                      r"row_flags_kernel|colsum(_q8)?_kernel|cast2d_kernel|sum_slabs_kernel|copy_rows_kernel|head_label_terms_kernel|"
                      r"dropout_mask_kernel)(<|$)")
F32 = np.float32


def f32(x):
    """float64 values exact in fp32"""
    return np.asarray(x, np.float64).astype(F32).astype(np.float64)


def _by(cases):
    d = {c["name"]: c for c in cases}
    assert len(d) == len(cases)
    return d


# ------------------------------------------------------------------------------------------------ im2col
# pad: ldp = ps*ps*3 + pad.  off: elements between a 16-B line and the window's first element (0: aligned)
IM2COL = [
    dict(name="i2c_2x64_p32", B=2, img=64, ps=32, pad=8, off=0, trunc=0),         # vector path (ps*3 = 96), ldp > K
    dict(name="i2c_1x48_p16", B=1, img=48, ps=16, pad=0, off=0, trunc=0),         # vector path, ldp = K, 9 patches
    dict(name="i2c_2x24_p4", B=2, img=24, ps=4, pad=0, off=0, trunc=0),           # element path: ps*3 = 12
    dict(name="i2c_1x48_p16_ldp4", B=1, img=48, ps=16, pad=4, off=0, trunc=0),    # element path through ldp % 8 != 0
    dict(name="i2c_1x48_p16_base8", B=1, img=48, ps=16, pad=8, off=1, trunc=0),   # element path through a window 8 B into a line
    dict(name="i2c_2x64_p32_trunc", B=2, img=64, ps=32, pad=8, off=0, trunc=1),   # vector path, trunc
    dict(name="i2c_2x24_p4_trunc", B=2, img=24, ps=4, pad=8, off=0, trunc=1),     # element path, trunc, ldp > K
]
IM2COL_BY = _by(IM2COL)


def im2col_off(c, dtype):
    """the Buf offset (elements) of the patches window: 16 B (32 B for fp32) into the allocation, or 8 B when misaligned"""
    return 8 if not c["off"] else (4 if dtype == "bf16" else 2)


def im2col_vec(c, dtype):
    """mic_im2col's `vec`: (ps*3) % 8 == 0, ldp % 8 == 0, both bases 16-B aligned, (img*3) % 4 == 0, fewer than 2^31 elements"""
    ldp = c["ps"] * c["ps"] * 3 + c["pad"]
    return (c["ps"] * 3) % 8 == 0 and ldp % 8 == 0 and not c["off"] and (c["img"] * 3) % 4 == 0 and c["B"] * c["img"] ** 2 * 3 < 2 ** 31


def im2col_kernels_of(c, dtype):
    return [f"im2col{'8' if im2col_vec(c, dtype) else ''}_kernel<{TN[dtype]}>"]


def im2col_inputs(c):
    """pixels [B][img][img][3], fp32 values.  trunc cases: negative fractions in (-1, 0) (every 7th element), values one ulp below
    an integer (every 11th), the rest uniform in (-2, 256)"""
    rng = np.random.default_rng(len(c["name"]) + c["img"])
    n = c["B"] * c["img"] ** 2 * 3
    if not c["trunc"]:
        return f32(rng.standard_normal(n) * 3).reshape(c["B"], c["img"], c["img"], 3)
    x = rng.uniform(-2, 256, n).astype(F32)
    x[::7] = -rng.uniform(0.001, 0.999, x[::7].size).astype(F32)
    k = rng.integers(1, 256, x[3::11].size).astype(F32)
    x[3::11] = np.nextafter(k, F32(0))
    return x.astype(np.float64).reshape(c["B"], c["img"], c["img"], 3)


# ------------------------------------------------------------------------------------------------ ViT assembly
VIT = [
    dict(name="vit_1x2x8", B=1, S=2, width=8, pad=0),          # the smallest: one class row, one patch row
    dict(name="vit_2x50x12", B=2, S=50, width=12, pad=4),      # width 12, ldp > width
    dict(name="vit_3x2x768", B=3, S=2, width=768, pad=8),      # S = 2 at the product's width
    dict(name="vit_2x50x8_ld", B=2, S=50, width=8, pad=24),    # width 8 under a wide row stride
    dict(name="vit_7x50x768", B=7, S=50, width=768, pad=0),    # 268 800 elements > 1024 * 256: the grid-stride trip
]
VIT_BY = _by(VIT)


def vit_inputs(c, dtype):
    rng = np.random.default_rng(c["B"] * 1000 + c["S"] + c["width"])
    B, S, W = c["B"], c["S"], c["width"]
    patch = round_to(rng.standard_normal((B * (S - 1), W)), dtype)
    return patch, f32(rng.standard_normal(W)), f32(rng.standard_normal((S, W)) * 0.5)


# B, S, width, pad; k = the longest chain of adds into an element of dpos / dcls (vit_bwd_k)
VIT_BWD = [
    dict(name="vitb_1x3x64", B=1, S=3, width=64, pad=0),       # bf16 vector kernel, 1 slice
    dict(name="vitb_9x3x64", B=9, S=3, width=64, pad=8),       # 4 slices of 3: the last one empty; ldp > width
    dict(name="vitb_33x2x16", B=33, S=2, width=16, pad=0),     # 8 slices of 5: slice 6 ragged (3 rows), slice 7 empty
    dict(name="vitb_2x50x768", B=2, S=50, width=768, pad=8),   # 4800 (s, chunk) pairs: more than one block
    dict(name="vitb_3x3x12", B=3, S=3, width=12, pad=0),       # bf16 element fallback: width % 8 != 0
    dict(name="vitb_3x3x16_ldp4", B=3, S=3, width=16, pad=4),  # bf16 element fallback: ldp % 8 != 0
]
VIT_BWD_BY = _by(VIT_BWD)


def vit_bwd_slices(c, dtype):
    """0: the element kernel; else gridDim.y of vit_assemble_bwd8_kernel (bf16, width % 8 == 0, ldp % 8 == 0, aligned bases)"""
    if dtype != "bf16" or c["width"] % 8 or (c["width"] + c["pad"]) % 8:
        return 0
    return 8 if c["B"] >= 32 else (4 if c["B"] >= 8 else 1)


def vit_bwd_k(c, dtype):
    """element kernel: B adds into the thread's sum (from 0) + 1 atomic.  Vector kernel: ceil(B / slices) adds + one atomic per slice"""
    s = vit_bwd_slices(c, dtype)
    return c["B"] + 1 if not s else -(-c["B"] // s) + s


def vit_bwd_kernels_of(c, dtype):
    return ["vit_assemble_bwd8_kernel"] if vit_bwd_slices(c, dtype) else [f"vit_assemble_bwd_kernel<{TN[dtype]}>"]


def start_values(rng, abs_sum):
    """non-zero start values of an accumulator fed by atomics, |start| <= min(1, sum |terms|) per element: the condition under which
    gamma_k(k) sum |terms| + U32 |start| bounds A atomics into it (util_scatter_ref.atomic_bound)"""
    u = rng.uniform(0.25, 1.0, abs_sum.shape) * rng.choice([-1.0, 1.0], abs_sum.shape)
    return f32(u * np.minimum(1.0, abs_sum) * 0.999)


def start_table(rng, abs_sum):
    """start values of a whole table: bounded as in start_values where terms arrive, of ordinary size in the rows nothing is added to"""
    return np.where(abs_sum > 0, start_values(rng, abs_sum), f32(rng.standard_normal(abs_sum.shape)))


def vit_bwd_inputs(c, dtype):
    rng = np.random.default_rng(c["B"] * 100 + c["S"] * 7 + c["width"])
    B, S, W = c["B"], c["S"], c["width"]
    dx = round_to(rng.standard_normal((B, S, W)), dtype)
    a = np.abs(dx).sum(0)
    return dx, start_values(rng, a), start_values(rng, a[0])


# ------------------------------------------------------------------------------------------------ token embedding
EMBED_FWD = [
    dict(name="emb_1x8", rows=1, width=8, V=5, P=4),             # one row, one chunk
    dict(name="emb_37x520", rows=37, width=520, V=50, P=40),     # 65 chunks a row
    dict(name="emb_37x1024", rows=37, width=1024, V=50, P=40),   # the product's width
    dict(name="emb_4100x1024", rows=4100, width=1024, V=64, P=40),  # 524 800 chunks > 2048 * 256: the grid-stride trip
]
EMBED_FWD_BY = _by(EMBED_FWD)
EMBED_SCALE = 32.0 * 0.37  # not a power of two: a * scale rounds


def embed_ids(c):
    """ids with 0 and V - 1, repeats; position ids with 0 and P - 1.  A table row / position row nobody names stays NaN"""
    rng = np.random.default_rng(c["rows"] + c["width"])
    rows, V, P = c["rows"], c["V"], c["P"]
    ids = rng.integers(0, max(V - 2, 1), rows)
    pos = rng.integers(0, P, rows)
    ids[0], pos[0] = V - 1, P - 1
    if rows > 4:
        ids[1], ids[2], ids[3], ids[-1] = 0, 3, 3, V - 1
        pos[1], pos[2], pos[-1] = 0, 0, P - 1
    return ids.astype(np.int32), pos.astype(np.int32)


def embed_fwd_inputs(c, dtype):
    rng = np.random.default_rng(c["rows"] * 3 + c["width"])
    ids, pos = embed_ids(c)
    table = np.full((c["V"], c["width"]), np.nan)
    u = np.unique(ids)
    table[u] = round_to(rng.standard_normal((u.size, c["width"])) * 0.05, dtype)
    ptab = np.full((c["P"] + 2, c["width"]), np.nan)   # rows 0 and 1 are never read: pos_ids + 2
    u = np.unique(pos) + 2
    ptab[u] = f32(rng.standard_normal((u.size, c["width"])))
    return ids, pos, table, ptab


# mode: which of dtable / dpos_table is given.  k (dtable) = occurrences of the id + 1 (the product dh * scale rounds, then one
# atomic add per occurrence); k (dpos) = occurrences of the position
EMBED_BWD = [
    dict(name="embb_37x64", rows=37, width=64, V=50, P=40, mode="both"),
    dict(name="embb_37x24_dtable", rows=37, width=24, V=50, P=40, mode="dtable"),   # dpos NULL; width 24: no vector assumption
    dict(name="embb_37x24_dpos", rows=37, width=24, V=50, P=40, mode="dpos"),       # dtable NULL
    dict(name="embb_1030x1024", rows=1030, width=1024, V=64, P=40, mode="both"),    # 1 054 720 elements > 4096 * 256: grid stride
]
EMBED_BWD_BY = _by(EMBED_BWD)


def embed_bwd_inputs(c, dtype):
    rng = np.random.default_rng(c["rows"] * 5 + c["width"])
    ids, pos = embed_ids(c)
    ids[::3] = 5   # one id on a third of the rows
    dh = round_to(rng.standard_normal((c["rows"], c["width"])), dtype)
    at, ap = np.zeros((c["V"], c["width"])), np.zeros((c["P"] + 2, c["width"]))
    np.add.at(at, ids, np.abs(dh) * float(F32(EMBED_SCALE)))
    np.add.at(ap, pos + 2, np.abs(dh))
    return ids, pos, dh, start_table(rng, at), start_table(rng, ap)


# ------------------------------------------------------------------------------------------------ deterministic scatter
# n rows, width, vocab.  neg: a third of the rows carry id -1 and a NaN dh row.  Planted ids (det_ids): see there
DET = [
    dict(name="det_1x64", n=1, width=64, vocab=7, neg=0),             # one row: det_single, count 1; lanes 1 .. 15 hold no column
    dict(name="det_5x64", n=5, width=64, vocab=9, neg=0),             # count 3 with its last occurrence in the scalar tail (n % 4 = 1), count 2
    dict(name="det_13x1088", n=13, width=1088, vocab=40, neg=0),      # counts 1 .. 4, second column block of 64 columns (one lane)
    dict(name="det_1100x1024", n=1100, width=1024, vocab=1500, neg=0),  # 35 bitmap words: the rotation acts at words 16 .. 34; one full block
    dict(name="det_1100x2048_neg", n=1100, width=2048, vocab=1500, neg=1),  # two full column blocks; a third of the rows skipped
    dict(name="det_1102x1088", n=1102, width=1088, vocab=1500, neg=0),  # a scalar tail of 2 behind 275 vector trips; partial second block
    dict(name="det_65536x64", n=65536, width=64, vocab=70000, neg=0, only="bf16"),  # the largest n: 2048 words, 8 KiB bitmap
]
DET_BY = _by(DET)


def det_ids(c, variant=0):
    """(ids, planted).  planted: {id: sorted positions}.  n = 1: one row.  n = 5: id 0 at (0, 2, 4), id vocab - 1 at (1, 3).  n = 13:
    counts 3, 2, 1, 4.  From 64 rows on: ids 0 and vocab - 1 carry 3 and 2 occurrences, ids 1, 5, 6 carry 1, 5, 9 at random places, id 3
    has its 4 occurrences inside bitmap word 0, id vocab - 2 fills word 1 (32 occurrences), id vocab - 3 has one occurrence in every
    one of min(words - 2, 40) words (bit (5 w) % 32 of word w = 2 ...).  Id 0 always owns position n - 1: the scalar tail of the scan
    when n % 4 != 0.  Every other row holds an id of its own.
    variant 1: the same planted positions, every other row a DIFFERENT id (the order is a function of the index set only)"""
    n, V = c["n"], c["vocab"]
    rng = np.random.default_rng(n + c["width"])
    ids = np.full(n, -2, np.int64)
    planted = {}

    def plant(i, pos):
        pos = sorted(int(p) for p in pos)
        assert all(ids[p] == -2 for p in pos), (i, pos)
        ids[pos] = i
        planted[i] = pos

    if n == 1:
        plant(V - 1, [0])
    elif n == 5:
        plant(0, [0, 2, 4])
        plant(V - 1, [1, 3])
    elif n == 13:
        plant(0, [1, 5, 12])
        plant(V - 1, [0, 7])
        plant(1, [3])
        plant(2, [2, 6, 8, 9])
    else:
        words = (n + 31) // 32
        plant(V - 2, range(32, 64))
        plant(V - 3, [w * 32 + (5 * w) % 32 for w in range(2, 2 + min(words - 2, 40))])
        plant(3, [8, 9, 17, 30])
        for cnt, i in ((3, 0), (2, V - 1), (1, 1), (5, 5), (9, 6)):
            free = np.flatnonzero(ids[:n - 1] == -2)
            plant(i, rng.choice(free, cnt - (i == 0), replace=False).tolist() + ([n - 1] if i == 0 else []))
    free = np.flatnonzero(ids == -2)
    pool = np.setdiff1d(np.arange(V), np.array(list(planted)))
    fill = np.random.default_rng(n + 1).permutation(pool)
    fill = fill[:free.size] if not variant else np.roll(fill, 1)[:free.size]
    assert fill.size == free.size
    ids[free] = fill
    if c["neg"]:
        taken = {p for v in planted.values() for p in v}
        ids[[p for p in range(1, n, 3) if p not in taken]] = -1
    return ids.astype(np.int32), planted


def det_inputs(c, dtype):
    """(dh with NaN rows where ids < 0, the start table with values in the rows some id names and in every 5th other row)"""
    rng = np.random.default_rng(c["n"] * 3 + c["width"])
    ids, _ = det_ids(c)
    dh = round_to(rng.standard_normal((c["n"], c["width"])), dtype)
    dh[ids < 0] = np.nan
    base = f32(rng.standard_normal((c["vocab"], c["width"])))
    return dh, base


# ------------------------------------------------------------------------------------------------ column sums
def ceil8(n):
    return (n + 7) // 8 * 8


# ld = ceil8(cols) + pad (pad % 8 == 0), columns cols .. ld hold NaN
COLSUM = [
    dict(name="cs_1x8", rows=1, cols=8, pad=0, acc=0),           # one row, one chunk: seven of eight row lanes idle
    dict(name="cs_7x204", rows=7, cols=204, pad=8, acc=0),       # a partial chunk (columns 200 .. 203), row lane 7 idle; NaN from column 204
    dict(name="cs_64x256", rows=64, cols=256, pad=8, acc=1),     # exactly one block, adds to a start vector
    dict(name="cs_65x264", rows=65, cols=264, pad=0, acc=0),     # gx = 2, gy = 2 (rows_per 33)
    dict(name="cs_65x204_acc", rows=65, cols=204, pad=16, acc=1),  # partial chunk with two row slices, accumulate
    dict(name="cs_8200x2048_cap", rows=8200, cols=2048, pad=0, acc=0, only="bf16"),  # ceil(8200 / 64) = 129 > cap 128: gy = 128, rows_per 65
]
COLSUM_BY = _by(COLSUM)
# nine items of different shapes in one grouped call: 8 + 1 = two launches
COLSUM_GROUP = [(1, 8), (7, 204), (64, 256), (65, 264), (130, 40), (9, 520), (3, 1032), (200, 16), (65, 204)]
COLSUM_Q8 = [
    dict(name="csq_1x8", rows=1, cols=8, pad=0),
    dict(name="csq_65x264", rows=65, cols=264, pad=8),           # gx = 2, gy = 2, ld > cols
    dict(name="csq_520x8", rows=520, cols=8, pad=8),             # every finite byte value in one column block, gy = 9
]
COLSUM_Q8_BY = _by(COLSUM_Q8)
COLSUM_Q8_GROUP = [(1, 8), (7, 200), (64, 256), (65, 264), (130, 40), (9, 520), (3, 1032), (200, 16), (65, 208)]
Q8_FMTS = ("e4m3", "e5m2")
Q8_SCALES = (0.25, 0.37)  # scale_inv: a power of two and one that is not


def colsum_plan(rows, cols):
    """(gx, gy, rows_per, k) of colsum_launch / mic_colsum_q8_grouped: gx = ceil(cols / 256), gy = ceil(rows / 64) capped at
    ceil(1024 / gx); k = ceil(rows_per / 8) adds in a row lane + 8 in the LDS combine + one atomic per row slice"""
    gx = (cols + 255) // 256
    gy = max(1, min((rows + 63) // 64, (1024 + gx - 1) // gx))
    rows_per = (rows + gy - 1) // gy
    return gx, gy, rows_per, -(-rows_per // 8) + 8 + gy


def colsum_inputs(rows, cols, dtype, seed=0):
    rng = np.random.default_rng(rows * 31 + cols + seed)
    x = round_to(rng.standard_normal((rows, cols)) + 0.25, dtype)
    return x, start_values(rng, np.abs(x).sum(0))


def q8_bytes(rows, cols, fmt, seed=0):
    """uint8 [rows][cols] of finite fp8 bytes.  Column 1 holds subnormals and zeros only (a kernel that flushes them gets that
    column wrong by all of its value); with at least 254 elements in the other columns every finite byte value occurs there"""
    from util_scatter_ref import Q8_TABLE

    fin = np.flatnonzero(np.isfinite(Q8_TABLE[fmt])).astype(np.uint8)
    sub = fin[(fin & (0x78 if fmt == "e4m3" else 0x7C)) == 0]
    rng = np.random.default_rng(rows * 13 + cols + seed)
    b = fin[rng.integers(0, fin.size, (rows, cols))]
    other = np.flatnonzero(np.arange(rows * cols) % cols != 1)
    if other.size >= fin.size:
        b.reshape(-1)[rng.permutation(other)[:fin.size]] = fin
    b[:, 1] = sub[rng.integers(0, sub.size, rows)]
    b[0, 1] = sub[1]   # (never all zeros)
    return b


def claimed_kernels():
    """every instantiation some case of this module claims to launch (the dispatch rules restated)"""
    k = set()
    for dt in DTYPES:
        t = TN[dt]
        k |= {x for c in IM2COL for x in im2col_kernels_of(c, dt)}
        k |= {x for c in VIT_BWD for x in vit_bwd_kernels_of(c, dt)}
        k |= {f"vit_assemble_kernel<{t}>", f"embed_fwd_kernel<{t}>", f"embed_bwd_kernel<{t}>", f"colsum_kernel<{t}>", f"copy_rows_kernel<{t}>",
              f"sum_slabs_kernel<{t}>"}
        k |= {f"det_single_kernel<{t}>", f"det_multi_kernel<{t}>"} if any(c.get("only", dt) == dt for c in DET) else set()
    k |= {x for p in CAST_PAIRS for x in cast_kernels_of(*p)}
    return k | {"det_owner_kernel", "det_reset_kernel", "colsum_q8_kernel", "row_flags_kernel", "head_label_terms_kernel", "dropout_mask_kernel"}


# ------------------------------------------------------------------------------------------------ casts
CAST_PAIRS = (("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("bf16", "bf16"))
CAST2D = dict(rows=5, cols=33, ld_src=40, ld_dst=48)
CAST_N = (2 ** 20 + 5, 2 ** 21 + 3)   # mic_cast: rows of 2^20 and a remainder launch of 5 / 3 elements
# fp32 bit patterns for the fp32 -> bf16 cast
CAST_SPECIAL = np.array([
    0x3F808000,  # 1 + 2^-8: a tie, down to the even 1.0
    0x3F818000,  # 1 + 3 * 2^-8: a tie, up to the even 1 + 2^-6
    0xBF808000, 0xBF818000,
    0x3F808001, 0x3F807FFF,  # one ulp either side of a tie
    0x7F7F7FFF,  # the largest fp32 that stays finite in bf16
    0x7F7F8000,  # rounds to +inf
    0xFF7F8000,  # rounds to -inf
    0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x80008001,  # fp32 subnormals (a tie to 0, a tie up, the largest, a negative one)
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,  # +-0, +-inf
    0x7FC00000,  # NaN
    0x7F800001,  # a NaN whose payload lies in the 16 bits the cast drops: must stay a NaN, not turn into inf
], dtype=np.uint32)
# bf16 bit patterns for the casts from bf16: subnormals, zeros, infinities, the largest finite
CAST_SPECIAL_BF16 = np.array([0x0001, 0x8001, 0x007F, 0x0080, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7F7F, 0xFF7F, 0x7FC0], dtype=np.uint16)


def cast_split(n):
    """mic_cast: [(rows, cols)] of its one or two mic_cast2d launches"""
    cols = min(n, 1 << 20)
    rows = n // cols
    rem = n - rows * cols
    return [(rows, cols)] + ([(1, rem)] if rem else [])


def cast_kernels_of(src, dst):
    return [f"cast2d_kernel<{TN[src]}, {TN[dst]}>"]


def cast_source_bits(n, src):
    """n source bit patterns: random finite values with the special patterns in front (and behind 2^20, in the remainder)"""
    rng = np.random.default_rng(n)
    if src == "f32":
        b = (rng.standard_normal(n) * 3).astype(F32).view(np.uint32)
        sp = CAST_SPECIAL
    else:
        b = ((rng.standard_normal(n) * 3).astype(F32).view(np.uint32) >> 16).astype(np.uint16)
        sp = CAST_SPECIAL_BF16
    m = min(n, sp.size)
    b[:m] = sp[:m]
    if n > (1 << 20):
        b[-3:] = sp[:3]
    return b


# ------------------------------------------------------------------------------------------------ slabs
SLABS = [
    dict(name="slab_1x3x8", n=1, rows=3, cols=8),           # one slab: 0 + s0
    dict(name="slab_2x5x24", n=2, rows=5, cols=24),
    dict(name="slab_7x5x24", n=7, rows=5, cols=24),
    dict(name="slab_2x2052x2048", n=2, rows=2052, cols=2048),  # 525 312 groups of 8 > 2048 * 256: the grid-stride trip
]
SLABS_BY = _by(SLABS)


def slab_inputs(c):
    """[n][rows][cols] fp32 values with cancellation between the slabs (the order of the adds shows)"""
    rng = np.random.default_rng(c["n"] * 11 + c["rows"])
    x = rng.standard_normal((c["n"], c["rows"], c["cols"])) * np.array([1.0, -1.0, 300.0, 1e-3, -300.0, 7.0, 0.1])[:c["n"], None, None]
    return f32(x)


# ------------------------------------------------------------------------------------------------ row copies
# width "min": one 16-B vector a row (8 bf16 / 4 fp32).  gather / scatter: src_idx / dst_idx given
COPY = [dict(name=f"copy_{w}_{'g' if g else ''}{'s' if s else ''}{'_ld' if pad else ''}", n=n, width=w, gather=g, scatter=s, pad=pad)
        for (n, w, pad) in ((5, "min", 0), (37, 1024, 0), (9, "min", 1)) for g in (0, 1) for s in (0, 1)]
COPY.append(dict(name="copy_2100x4096", n=2100, width=4096, gather=1, scatter=1, pad=0, only="bf16"))  # 1 075 200 vectors > 4096 * 256
COPY_BY = _by(COPY)


def copy_width(c, dtype):
    return (8 if dtype == "bf16" else 4) if c["width"] == "min" else c["width"]


def copy_indices(c):
    """(src_idx with repeats into n + 3 source rows, dst_idx a permutation into n + 4 destination rows) or None"""
    rng = np.random.default_rng(c["n"])
    n = c["n"]
    si = rng.integers(0, n + 3, n)
    if n > 2:
        si[1] = si[0]
    di = rng.permutation(n + 4)[:n]
    return (si.astype(np.int32) if c["gather"] else None), (di.astype(np.int32) if c["scatter"] else None)


# ------------------------------------------------------------------------------------------------ row flags, label terms, mask
ROW_FLAGS = (1, 7, 250054)   # n_rows


def row_flag_ids(n_rows):
    """ids inside [0, n_rows) with repeats, plus ids < 0 and >= n_rows, which are ignored"""
    rng = np.random.default_rng(n_rows)
    ids = rng.integers(0, n_rows, 300)
    ids[:6] = [-1, n_rows, n_rows + 5, -(2 ** 31), 2 ** 31 - 1, n_rows - 1]
    ids[6], ids[7] = 0, 0
    ids[50:60] = ids[40:50]
    return ids.astype(np.int32)


# pads: lde, ldh, ldx, ldde beyond width (lde, ldh multiples of 8, ldx of 4)
LABEL_TERMS = [
    dict(name="hlt_5x8", rows=5, width=8, V=6, pads=(0, 0, 0, 0)),
    dict(name="hlt_9x1024", rows=9, width=1024, V=12, pads=(8, 16, 4, 3)),   # four column trips of the 256 threads; every ld wider
    dict(name="hlt_300x264", rows=300, width=264, V=12, pads=(8, 8, 8, 8)),  # labels shared by ~25 rows: long atomic chains
]
LABEL_TERMS_BY = _by(LABEL_TERMS)


def label_terms_inputs(c):
    """labels shared by several rows (and one label only a coef == 0 row names), coef with exact zeros, bf16 E and h"""
    rng = np.random.default_rng(c["rows"] + c["width"])
    rows, W, V = c["rows"], c["width"], c["V"]
    labels = rng.integers(0, V - 2, rows)
    labels[0] = labels[1] = labels[-1] = 2
    coef = f32(rng.standard_normal(rows) * 0.1)
    coef[1::4] = 0.0
    labels[1] = V - 1   # named only by a row whose coef is 0: dE[V - 1] stays as it was, E[V - 1] is not read
    E = round_to(rng.standard_normal((V, W)), "bf16")
    E[V - 1] = np.nan
    h = round_to(rng.standard_normal((rows, W)), "bf16")
    h[coef == 0] = np.nan   # a row with coef == 0 reads neither E nor h
    a = np.zeros((V, W))
    live = coef != 0
    np.add.at(a, labels[live], np.abs(coef[live, None] * h[live]))
    return labels.astype(np.int32), coef, E, h, start_table(rng, a)


DROPOUT_N = 262144 + 5   # one more than 1024 * 256 threads: the grid stride
DROPOUT_P = (0.0, 0.1, 0.5)
