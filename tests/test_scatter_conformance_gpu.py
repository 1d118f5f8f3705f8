"""Gather / scatter conformance on the MI355X: the embeddings, the ViT assembly, the column sums and the small data-movement
kernels of csrc/elementwise.hip (33 instantiations) on every case of tests/util_scatter_cases.py, in bf16 and fp32 where the
entry point takes a dtype, against the references and derived bounds of tests/util_scatter_ref.py.  Around every call:
  - outputs are windows in canary-filled allocations (extra rows, a row stride wider than the columns where the entry point takes
    one, a base 16 B into the allocation); every element outside the window keeps its bits;
  - what a kernel must not read holds NaN: columns cols .. ld, rows past the count, the dh rows of ids < 0, table rows no id names,
    the E / h rows of a coef == 0 label term;
  - every launch whose result does not pass through fp32 atomics runs twice and gives identical bits; accumulators are restored
    between the runs.
Pure data movement is compared exactly, one-rounding kernels and the sums under their bounds (`check`), the fixed-order sums
(mic_sum_slabs, dx_slab of mic_head_label_terms, mic_embed_rows_add_det) also bit for bit with their numpy emulation.
Out of scope: mic_fp8_quantize / mic_fp8_amax / mic_fp8_roll_amax (byte-exact against torch in tests/test_fp8_gpu.py),
mic_image_transform, the decode epilogues, mic_comm_emulate and the stream helpers."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_scatter_cases as SC  # noqa: E402
import util_scatter_ref as SR  # noqa: E402
from test_attn_conformance_gpu import IB, TD, Buf, _refused  # noqa: E402
from test_rowop_conformance_gpu import ints, twice, vec, zero_bits  # noqa: E402
from util_gemm_ref import check, check_canary, round_to  # noqa: E402
from util_rowop_ref import keep_mask  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32
BF = torch.bfloat16
Q8T = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}


def dtypes_of(c):
    return [c["only"]] if c.get("only") else list(SC.DTYPES)


def cases(table):
    return [(c["name"], dt) for c in table for dt in dtypes_of(c)]


def same_values(got, ref, what):
    """exact as values (+0 == -0), no NaN on either side"""
    assert np.array_equal(got, ref), f"{what}: {int((got != ref).sum())} element(s) differ, first at {np.argwhere(got != ref)[0].tolist()}"


def same_bits(got, emu, what):
    """float64 views of fp32 / bf16 results: the same bits, the sign of a zero included"""
    g, e = np.asarray(got, np.float64), np.asarray(emu, np.float64)
    assert np.array_equal(g, e) and np.array_equal(np.signbit(g), np.signbit(e)), \
        f"{what}: {int((g != e).sum())} element(s) differ from the emulation's bits"


def mat(x, dt, dev, fill="nan", pad=0, off=8, extra=3):
    """float64 [rows][cols] -> a Buf window with row stride cols + pad"""
    return Buf(x.shape[0], x.shape[1], x.shape[1] + pad, dt, dev, fill, off=off, extra=extra).put(x)


class Bytes:
    """a window of n bytes 16 B into a uint8 allocation filled with `fill`, 48 B behind it"""

    def __init__(self, n, dev, fill=0xA5):
        self.n, self.fill = n, fill
        self.flat = torch.empty(n + 64, dtype=torch.uint8, device=dev)
        self.t = self.flat[16:16 + n]
        self.refill()

    def refill(self):
        self.flat.fill_(self.fill)

    def check_canary(self, what):
        check_canary(self.flat, (slice(16, 16 + self.n),), what)


# ------------------------------------------------------------------------------------------------ im2col
@pytest.mark.parametrize("name,dtype", cases(SC.IM2COL))
def test_im2col(dev, name, dtype):
    from mic_amd import ops

    c, dt = SC.IM2COL_BY[name], TD[dtype]
    B, img, ps = c["B"], c["img"], c["ps"]
    K, rows = ps * ps * 3, B * (img // ps) ** 2
    px = SC.im2col_inputs(c)
    pd = Buf(B * img * img, 3, 3, F32, dev, "nan").put(px.reshape(-1, 3))
    assert pd.t.data_ptr() % 16 == 0
    out = Buf(rows, K, K + c["pad"], dt, dev, "canary", off=SC.im2col_off(c, dtype))
    assert (out.t.data_ptr() % 16 == 0) == (not c["off"])
    twice(lambda: ops.im2col(pd.t, out.t, B, img, ps, out.ld, trunc_int32=bool(c["trunc"])), [out], name)
    out.check_canary(name)
    got = out.get()
    same_values(got, SR.im2col_ref(px, B, img, ps, c["trunc"], dtype), f"im2col/{dtype} {name}")
    if c["trunc"]:  # what trunc leaves of a pixel in (-1, 0): -0.0, where the cast through int32 gives +0.0 (equal as values)
        neg = SR.im2col_ref(((px > -1) & (px < 0)).astype(np.float64), B, img, ps, 0, dtype) != 0
        assert neg.any() and np.signbit(got[neg]).all() and not got[neg].any(), f"{name}: trunc of a pixel in (-1, 0) is not -0.0"


# ------------------------------------------------------------------------------------------------ ViT assembly
@pytest.mark.parametrize("name,dtype", cases(SC.VIT))
def test_vit_assemble(dev, name, dtype):
    from mic_amd import ops

    c, dt = SC.VIT_BY[name], TD[dtype]
    B, S, W = c["B"], c["S"], c["width"]
    patch, cls, pos = SC.vit_inputs(c, dtype)
    pb = mat(patch, dt, dev, pad=c["pad"])
    cb, sb = vec(W, dev, "nan").put(cls[None]), mat(pos, F32, dev, off=4)
    x = Buf(B * S, W, W, dt, dev, "canary")
    twice(lambda: ops.vit_assemble(pb.t, cb.t[0], sb.t, x.t, B, S, W, pb.ld), [x], name)
    x.check_canary(name)
    ref, bound = SR.vit_assemble_ref(patch, cls, pos, B, S, dtype)
    check(x.get(), ref, bound, f"vit_assemble/{dtype} x: {name}")


@pytest.mark.parametrize("name,dtype", cases(SC.VIT_BWD))
def test_vit_assemble_bwd(dev, name, dtype):
    """dpatch exact; dpos / dcls (fp32 atomics) from non-zero start values under the bound with k = SC.vit_bwd_k"""
    from mic_amd import ops

    c, dt = SC.VIT_BWD_BY[name], TD[dtype]
    B, S, W = c["B"], c["S"], c["width"]
    dx, dpos0, dcls0 = SC.vit_bwd_inputs(c, dtype)
    dxb = mat(dx.reshape(B * S, W), dt, dev)
    dp = Buf(B * (S - 1), W, W + c["pad"], dt, dev, "canary")
    dpos, dcls = Buf(S, W, W, F32, dev, "canary", off=4), vec(W, dev)
    twice(lambda: ops.vit_assemble_bwd(dxb.t, dp.t, dcls.t[0], dpos.t, B, S, W, dp.ld), [dp, dpos, dcls], name,
          prep=lambda: (dpos.put(dpos0), dcls.put(dcls0[None])), inexact=[dpos, dcls])
    for o in (dp, dpos, dcls):
        o.check_canary(name)
    r_dp, (r_pos, e_pos), (r_cls, e_cls) = SR.vit_bwd_ref(dx, dpos0, dcls0, SC.vit_bwd_k(c, dtype))
    same_values(dp.get(), r_dp, f"vit_assemble_bwd/{dtype} dpatch {name}")
    check(dpos.get(), r_pos, e_pos, f"vit_assemble_bwd/{dtype} dpos: {name}")
    check(dcls.get()[0], r_cls, e_cls, f"vit_assemble_bwd/{dtype} dcls: {name}")


# ------------------------------------------------------------------------------------------------ token embedding
@pytest.mark.parametrize("name,dtype", cases(SC.EMBED_FWD))
def test_embed_fwd(dev, name, dtype):
    from mic_amd import ops

    c, dt = SC.EMBED_FWD_BY[name], TD[dtype]
    rows, W = c["rows"], c["width"]
    ids, pos, table, ptab = SC.embed_fwd_inputs(c, dtype)
    tb, pb = mat(table, dt, dev), mat(ptab, F32, dev, off=4)
    h = Buf(rows, W, W, dt, dev, "canary")
    idd, pd = ints(ids, dev), ints(pos, dev)
    twice(lambda: ops.embed_fwd(idd, pd, tb.t, pb.t, SC.EMBED_SCALE, h.t, rows, W), [h], name)
    h.check_canary(name)
    ref, bound = SR.embed_fwd_ref(ids, pos, table, ptab, SC.EMBED_SCALE, dtype)
    check(h.get(), ref, bound, f"embed_fwd/{dtype} h: {name}")


@pytest.mark.parametrize("name,dtype", cases(SC.EMBED_BWD))
def test_embed_bwd(dev, name, dtype):
    from mic_amd import ops

    c, dt = SC.EMBED_BWD_BY[name], TD[dtype]
    rows, W, V, P2 = c["rows"], c["width"], c["V"], c["P"] + 2
    ids, pos, dh, dt0, dp0 = SC.embed_bwd_inputs(c, dtype)
    dhb = mat(dh, dt, dev)
    dtb, dpb = Buf(V, W, W, F32, dev, "canary", off=4), Buf(P2, W, W, F32, dev, "canary", off=4)
    idd, pd = ints(ids, dev), ints(pos, dev)
    use_t, use_p = c["mode"] != "dpos", c["mode"] != "dtable"
    twice(lambda: ops.embed_bwd(idd if use_t else None, pd if use_p else None, dhb.t, SC.EMBED_SCALE, dtb.t if use_t else None,
                                dpb.t if use_p else None, rows, W), [dtb, dpb], name,
          prep=lambda: (dtb.put(dt0), dpb.put(dp0)), inexact=[dtb, dpb])
    dtb.check_canary(name)
    dpb.check_canary(name)
    (r_t, e_t), (r_p, e_p) = SR.embed_bwd_ref(ids, pos, dh, SC.EMBED_SCALE, V, P2, dt0, dp0)
    if use_t:
        check(dtb.get(), r_t, e_t, f"embed_bwd/{dtype} dtable: {name}")
    else:
        same_values(dtb.get(), dt0, f"{name}: a NULL dtable's neighbour")
    if use_p:
        check(dpb.get(), r_p, e_p, f"embed_bwd/{dtype} dpos_table: {name}")
    else:
        same_values(dpb.get(), dp0, f"{name}: a NULL dpos_table's neighbour")


# ------------------------------------------------------------------------------------------------ deterministic scatter
def _det_run(ops, c, dtype, dev, ids, dh, base, scale, ws=None):
    """one call from a fresh table: (table Buf, workspace, its state before the call)"""
    dt = TD[dtype]
    dhb = mat(dh, dt, dev)
    tb = Buf(c["vocab"], c["width"], c["width"], F32, dev, "canary", off=4).put(base)
    ws = ops.embed_rows_add_det_workspace(c["vocab"], dev) if ws is None else ws
    ws0 = ws.clone()
    idd = ints(ids, dev)
    assert idd.data_ptr() % 16 == 0 and dhb.t.data_ptr() % 16 == 0
    ops.embed_rows_add_det(idd, dhb.t, scale, tb.t, c["n"], c["width"], ws)
    torch.cuda.synchronize()
    return tb, ws, ws0


@pytest.mark.parametrize("name,dtype", cases(SC.DET))
def test_embed_rows_add_det(dev, name, dtype):
    """the three levels: (1) fp64 under gamma_k(count + 2) scale sum |dh| + U32 |base| with scale 0.37; (2) bit for bit the
    documented order (SR.emu_det) with scale 0.5 and 32; (3) the header's promises: the workspace's first 3 vocab + 1 ints as
    found, rows no id names untouched, a second call on the same workspace gives the same bits, and the bits of a row depend only on
    where its id occurs"""
    from mic_amd import ops

    c = SC.DET_BY[name]
    V = c["vocab"]
    ids, planted = SC.det_ids(c)
    dh, base = SC.det_inputs(c, dtype)
    named = np.zeros(V, bool)
    named[ids[ids >= 0]] = True
    # level 1
    tb, ws, ws0 = _det_run(ops, c, dtype, dev, ids, dh, base, 0.37)
    tb.check_canary(name)
    ref, bound = SR.det_ref(ids, np.nan_to_num(dh), 0.37, base)
    got = tb.get()
    check(got[named], ref[named], bound[named], f"embed_rows_add_det/{dtype} dtable scale 0.37: {name}")
    same_bits(got[~named], base[~named], f"{name}: table rows no id names")
    assert torch.equal(ws[:3 * V + 1], ws0[:3 * V + 1]), f"{name}: the workspace's first 3 vocab + 1 ints are not as found"
    # level 2, and the second call on the workspace the first call left
    for scale in (0.5, 32.0):
        emu = SR.emu_det(ids, dh, scale, base).astype(np.float64)
        t1, ws, _ = _det_run(ops, c, dtype, dev, ids, dh, base, scale, ws)
        same_bits(t1.get(), emu, f"embed_rows_add_det/{dtype} scale {scale}: {name}")
        t2, ws2, _ = _det_run(ops, c, dtype, dev, ids, dh, base, scale)
        assert torch.equal(t1.bits(), t2.bits()), f"{name}: a used workspace and a fresh one give different bits"
        assert torch.equal(ws[:3 * V + 1], ws0[:3 * V + 1])
    # level 3: other ids everywhere else (and other dh rows there), the planted ids where they were
    ids2, planted2 = SC.det_ids(c, variant=1)
    assert planted2 == planted
    keep = np.zeros(c["n"], bool)
    keep[[p for v in planted.values() for p in v]] = True
    assert not (ids2[~keep & (ids >= 0)] == ids[~keep & (ids >= 0)]).any()
    dh2 = np.where(keep[:, None], dh, round_to(np.nan_to_num(dh) * 1.5 + 0.25, dtype))
    dh2[ids2 < 0] = np.nan
    t3, _, _ = _det_run(ops, c, dtype, dev, ids2, dh2, base, 32.0, ws)
    rows = sorted(planted)
    assert np.array_equal(t3.get()[rows], t1.get()[rows]), f"{name}: the bits of a row changed with the OTHER ids of the call"


# ------------------------------------------------------------------------------------------------ column sums
def _colsum_item(rows, cols, pad, dtype, dev, seed=0):
    x, start = SC.colsum_inputs(rows, cols, dtype, seed)
    xb = Buf(rows, cols, SC.ceil8(cols) + pad, TD[dtype], dev, "nan").put(x)
    return x, start, xb, vec(cols, dev)


@pytest.mark.parametrize("name,dtype", cases(SC.COLSUM))
def test_colsum(dev, name, dtype):
    from mic_amd import ops

    c = SC.COLSUM_BY[name]
    rows, cols = c["rows"], c["cols"]
    x, start, xb, out = _colsum_item(rows, cols, c["pad"], dtype, dev)
    k = SC.colsum_plan(rows, cols)[3]
    twice(lambda: ops.colsum(xb.t, out.t[0], rows, cols, xb.ld, accumulate=bool(c["acc"])), [out], name,
          prep=(lambda: out.put(start[None])) if c["acc"] else None, inexact=[out])
    out.check_canary(name)
    ref, bound = SR.colsum_ref(x, k, start if c["acc"] else None)
    check(out.get()[0], ref, bound, f"colsum/{dtype} out: {name}")


@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_colsum_grouped(dev, dtype):
    """nine items of different shapes: two launches, every item accumulates into its own start vector"""
    from mic_amd import ops

    its = [_colsum_item(r, c, 8 * (i % 3), dtype, dev, seed=i) for i, (r, c) in enumerate(SC.COLSUM_GROUP)]
    outs = [t[3] for t in its]
    twice(lambda: ops.colsum_grouped([(xb.t, o.t[0], r, c, xb.ld) for (_, _, xb, o), (r, c) in zip(its, SC.COLSUM_GROUP)]), outs,
          "colsum_grouped", prep=lambda: [o.put(s[None]) for _, s, _, o in its], inexact=outs)
    for (x, start, _, o), (r, c) in zip(its, SC.COLSUM_GROUP):
        o.check_canary(f"colsum_grouped {r}x{c}")
        ref, bound = SR.colsum_ref(x, SC.colsum_plan(r, c)[3], start)
        check(o.get()[0], ref, bound, f"colsum_grouped/{dtype} out: {r}x{c}")


def _q8_item(rows, cols, pad, fmt, dev, seed=0):
    """fp8 bytes in a NaN-filled (0x7F is a NaN in both formats) allocation, row stride cols + pad"""
    b = SC.q8_bytes(rows, cols, fmt, seed)
    ld = cols + pad
    flat = torch.full((16 + (rows + 2) * ld,), 0x7F, dtype=torch.uint8, device=dev)
    win = flat[16:16 + rows * ld].view(rows, ld)[:, :cols]
    win.copy_(torch.from_numpy(b).to(dev))
    return b, win.view(Q8T[fmt]), flat


@pytest.mark.parametrize("scale_inv", SC.Q8_SCALES)
@pytest.mark.parametrize("fmt", SC.Q8_FMTS)
@pytest.mark.parametrize("name", [c["name"] for c in SC.COLSUM_Q8])
def test_colsum_q8(dev, name, fmt, scale_inv):
    from mic_amd import ops

    c = SC.COLSUM_Q8_BY[name]
    rows, cols = c["rows"], c["cols"]
    b, xq, _flat = _q8_item(rows, cols, c["pad"], fmt, dev)
    sinv = torch.tensor([scale_inv], dtype=F32, device=dev)
    k = SC.colsum_plan(rows, cols)[3]
    rng = np.random.default_rng(rows + cols)
    start = SC.start_values(rng, np.abs(SR.q8_decode(b, fmt)).sum(0) * scale_inv)
    out = vec(cols, dev)
    twice(lambda: ops.colsum_q8_grouped([(xq, out.t[0], sinv, rows, cols)]), [out], name, prep=lambda: out.put(start[None]), inexact=[out])
    out.check_canary(name)
    ref, bound = SR.colsum_q8_ref(b, fmt, scale_inv, k, start)
    check(out.get()[0], ref, bound, f"colsum_q8/f32 out {fmt}: {name} scale_inv {scale_inv}")


@pytest.mark.parametrize("fmt", SC.Q8_FMTS)
def test_colsum_q8_grouped(dev, fmt):
    from mic_amd import ops

    its, items = [], []
    for i, (r, c) in enumerate(SC.COLSUM_Q8_GROUP):
        b, xq, flat = _q8_item(r, c, 8 * (i % 3), fmt, dev, seed=i)
        sc = SC.Q8_SCALES[i % 2] * (1 + i)
        sinv = torch.tensor([sc], dtype=F32, device=dev)
        start = SC.start_values(np.random.default_rng(i), np.abs(SR.q8_decode(b, fmt)).sum(0) * sc)
        o = vec(c, dev)
        its.append((b, sc, start, o, flat, sinv))
        items.append((xq, o.t[0], sinv, r, c))
    outs = [t[3] for t in its]
    twice(lambda: ops.colsum_q8_grouped(items), outs, "colsum_q8_grouped", prep=lambda: [t[3].put(t[2][None]) for t in its], inexact=outs)
    for (b, sc, start, o, _, _), (r, c) in zip(its, SC.COLSUM_Q8_GROUP):
        o.check_canary(f"colsum_q8_grouped {r}x{c}")
        ref, bound = SR.colsum_q8_ref(b, fmt, sc, SC.colsum_plan(r, c)[3], start)
        check(o.get()[0], ref, bound, f"colsum_q8_grouped/f32 out {fmt}: {r}x{c}")


# ------------------------------------------------------------------------------------------------ casts
def _bits_tensor(bits, dtype, dev):
    t = torch.from_numpy(bits.view(np.int32 if dtype == "f32" else np.int16).copy()).to(dev)
    return t.view(TD[dtype])


def _bits_numpy(t):
    a = t.contiguous().view(IB[t.dtype]).cpu().numpy()
    return a.view(np.uint32 if t.dtype == F32 else np.uint16)


def _check_cast(got_bits, src_bits, src, dst, what):
    exp, nan = SR.cast_expected_bits(src_bits, src, dst)
    ok = got_bits[~nan] == exp[~nan]
    assert ok.all(), f"{what}: {int((~ok).sum())} element(s) differ, first source bits {hex(int(src_bits[~nan][~ok][0]))} -> {hex(int(got_bits[~nan][~ok][0]))}"
    g = got_bits[nan].astype(np.uint32) << (0 if dst == "f32" else 16)
    assert np.isnan(g.view(np.float32)).all(), f"{what}: a NaN did not stay a NaN"


@pytest.mark.parametrize("src,dst", SC.CAST_PAIRS)
def test_cast2d(dev, src, dst):
    """ld_src and ld_dst wider than cols; the special operands (ties both ways, the overflow edge, subnormals, +-0, +-inf, NaN)"""
    from mic_amd import ops

    rows, cols, lds, ldd = (SC.CAST2D[k] for k in ("rows", "cols", "ld_src", "ld_dst"))
    sb = SC.cast_source_bits(rows * cols, src).reshape(rows, cols)
    s = Buf(rows, cols, lds, TD[src], dev, "nan")
    s.t.copy_(_bits_tensor(sb, src, dev))
    d = Buf(rows, cols, ldd, TD[dst], dev, "canary")
    twice(lambda: ops.cast2d(s.t, d.t, rows, cols, lds, ldd), [d], f"cast2d {src}->{dst}")
    d.check_canary(f"cast2d {src}->{dst}")
    _check_cast(_bits_numpy(d.t), sb, src, dst, f"cast2d {src}->{dst}")


@pytest.mark.parametrize("n,src,dst", [(SC.CAST_N[0],) + p for p in SC.CAST_PAIRS] + [(SC.CAST_N[1], "f32", "bf16")])
def test_cast_flat(dev, n, src, dst):
    """mic_cast past 2^20 elements: rows of 2^20 and the remainder launch"""
    from mic_amd import ops

    assert len(SC.cast_split(n)) == 2
    sb = SC.cast_source_bits(n, src)
    s = Buf(1, n, n, TD[src], dev, "nan", extra=0)
    s.t[0].copy_(_bits_tensor(sb, src, dev))
    d = Buf(1, n, n, TD[dst], dev, "canary", extra=0)
    twice(lambda: ops.cast(s.t[0], d.t[0], n), [d], f"cast {n}")
    d.check_canary(f"cast {src}->{dst} {n}")
    _check_cast(_bits_numpy(d.t[0]), sb, src, dst, f"cast {src}->{dst} {n}")


# ------------------------------------------------------------------------------------------------ slabs
@pytest.mark.parametrize("dtype", SC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in SC.SLABS])
def test_sum_slabs(dev, name, dtype):
    """ld_src = cols + 4, slab_stride = rows * ld_src + 8 (NaN in between); bit for bit 0 + s0 + s1 + ... and under the fp64 bound"""
    from mic_amd import ops

    c, dt = SC.SLABS_BY[name], TD[dtype]
    n, rows, cols = c["n"], c["rows"], c["cols"]
    x = SC.slab_inputs(c)
    lds = cols + 4
    stride = rows * lds + 8
    flat = torch.full((4 + n * stride + 8,), float("nan"), dtype=F32, device=dev)
    for s in range(n):
        flat[4 + s * stride:4 + s * stride + rows * lds].view(rows, lds)[:, :cols] = torch.from_numpy(x[s]).to(dev).to(F32)
    src = flat[4:]
    out = Buf(rows, cols, cols + 8, dt, dev, "canary")
    twice(lambda: ops.sum_slabs(src, n, stride, out.t, rows, cols, lds, out.ld), [out], name)
    out.check_canary(name)
    got = out.get()
    same_bits(got, SR.emu_sum_slabs(x, dtype), f"sum_slabs/{dtype} {name}")
    ref, bound = SR.sum_slabs_ref(x, dtype)
    check(got, ref, bound, f"sum_slabs/{dtype} dst: {name}")


# ------------------------------------------------------------------------------------------------ row copies
@pytest.mark.parametrize("name,dtype", cases(SC.COPY))
def test_copy_rows(dev, name, dtype):
    from mic_amd import ops

    c, dt = SC.COPY_BY[name], TD[dtype]
    n, W = c["n"], SC.copy_width(c, dtype)
    pad = (8 if dtype == "bf16" else 4) * c["pad"]
    si, di = SC.copy_indices(c)
    rng = np.random.default_rng(n + W)
    x = round_to(rng.standard_normal((n + 3, W)), dtype)
    read = np.zeros(n + 3, bool)
    read[si if si is not None else np.arange(n)] = True
    x[~read] = np.nan   # source rows no index names
    sb = Buf(n + 3, W, W + pad, dt, dev, "nan", extra=0).put(x)
    db = Buf(n + 4, W, W + 2 * pad, dt, dev, "canary", extra=1)
    sid, did = (ints(i, dev) if i is not None else None for i in (si, di))
    twice(lambda: ops.copy_rows(sb.t, db.t, n, W, src_idx=sid, dst_idx=did), [db], name)
    rs, rd = (si if si is not None else np.arange(n)), (di if di is not None else np.arange(n))
    written = torch.zeros(n + 4, W, dtype=torch.bool)
    written[torch.from_numpy(rd.astype(np.int64))] = True
    db.check_canary(name, written)
    same_values(db.get()[rd], x[rs], f"copy_rows/{dtype} {name}")


# ------------------------------------------------------------------------------------------------ row flags, label terms, mask
@pytest.mark.parametrize("n_rows", SC.ROW_FLAGS)
def test_row_flags(dev, n_rows):
    """ids < 0 and >= n_rows are ignored, repeats are harmless; the n_ids .. entries of the id array hold an id that would show"""
    from mic_amd import ops

    ids = SC.row_flag_ids(n_rows)
    idd = ints(np.concatenate([ids, np.zeros(8, np.int32) + (n_rows - 1) // 2]), dev)
    if n_rows > 2:
        ids = np.where(ids == (n_rows - 1) // 2, 0, ids)
        idd[:ids.size] = torch.from_numpy(ids).to(dev)
    fl = Bytes(n_rows, dev)
    first = None
    for _ in range(2):
        fl.refill()
        ops.row_flags(idd, ids.size, fl.t)
        torch.cuda.synchronize()
        first = fl.flat.clone() if first is None else first
    assert torch.equal(fl.flat, first)
    fl.check_canary(f"row_flags {n_rows}")
    ref = np.zeros(n_rows, np.uint8)
    ref[ids[(ids >= 0) & (ids < n_rows)]] = 1
    assert np.array_equal(fl.t.cpu().numpy(), ref), f"row_flags {n_rows}"


@pytest.mark.parametrize("name", [c["name"] for c in SC.LABEL_TERMS])
def test_head_label_terms(dev, name):
    """dx_slab bit for bit np.float32(c) * np.float32(E) and under its fp64 bound, +0 bits in the rows with coef == 0; dE under the
    bound of its atomics, the rows no live label names untouched"""
    from mic_amd import ops

    c = SC.LABEL_TERMS_BY[name]
    rows, W, V = c["rows"], c["width"], c["V"]
    labels, coef, E, h, dE0 = SC.label_terms_inputs(c)
    Eb, hb = mat(E, BF, dev, pad=c["pads"][0]), mat(h, BF, dev, pad=c["pads"][1])
    dxb = Buf(rows, W, W + c["pads"][2], F32, dev, "canary", off=4)
    dEb = Buf(V, W, W + c["pads"][3], F32, dev, "canary", off=4)
    ld_, cd = ints(labels, dev), vec(rows, dev, "nan").put(coef[None])
    twice(lambda: ops.head_label_terms(ld_, cd.t[0], Eb.t, hb.t, dxb.t, dEb.t, rows, W), [dxb, dEb], name,
          prep=lambda: dEb.put(dE0), inexact=[dEb])
    dxb.check_canary(name)
    dEb.check_canary(name)
    r_dx, e_dx, r_dE, e_dE = SR.label_terms_ref(labels, coef, E, h, dE0)
    emu_dx, _ = SR.emu_label_terms(labels, coef, E, h, dE0)
    got = dxb.get()
    same_bits(got, emu_dx, f"head_label_terms dx_slab {name}")
    check(got, r_dx, e_dx + 1e-300, f"head_label_terms/bf16 dx_slab: {name}")
    dead = torch.from_numpy(coef == 0).to(dev)
    assert dead.any() and zero_bits(dxb.t[dead]), f"{name}: the dx_slab row of a coef == 0 row is not +0 bits"
    gE = dEb.get()
    check(gE, r_dE, e_dE, f"head_label_terms/bf16 dE: {name}")
    live = np.zeros(V, bool)
    live[labels[coef != 0]] = True
    assert not live[V - 1]
    same_bits(gE[~live], dE0[~live], f"{name}: dE rows no live label names")


@pytest.mark.parametrize("p", SC.DROPOUT_P)
def test_dropout_mask(dev, p):
    from mic_amd import _lib as L

    n = SC.DROPOUT_N
    m = Bytes(n, dev)
    first = None
    for _ in range(2):
        m.refill()
        L.check(L.lib().mic_dropout_mask(m.t.data_ptr(), n, float(p), 77, None), "mic_dropout_mask")
        torch.cuda.synchronize()
        first = m.flat.clone() if first is None else first
    assert torch.equal(m.flat, first)
    m.check_canary(f"dropout_mask p={p}")
    got = m.t.cpu().numpy()
    assert np.array_equal(got.astype(bool), keep_mask(n, p, 77)) and got.max() <= 1
    assert p > 0 or got.all()


# ------------------------------------------------------------------------------------------------ refusals
def test_scatter_refusals(dev):
    """every requirement the header states for the entry points in scope: MIC_EINVAL, the canary-filled outputs untouched — and for
    the deterministic scatter the workspace too: the next valid call on it gives the right bits"""
    from mic_amd import _lib as L
    from mic_amd import ops

    lib = L.lib()
    ones = lambda r, c, dt=BF, pad=0: mat(np.ones((r, c)), dt, dev, pad=pad)  # noqa: E731
    can = lambda r, c, dt=BF, pad=0, off=8: Buf(r, c, c + pad, dt, dev, "canary", off=off)  # noqa: E731
    P = lambda t: t.data_ptr()  # noqa: E731
    i4 = ints(np.zeros(4), dev)
    # im2col: img % ps, a storage type the library does not know
    px, out = ones(48 * 48, 3, F32), can(9, 768)
    _refused(lambda: ops.im2col(px.t, out.t, 1, 48, 18, out.ld), [out], "im2col img % ps")
    _refused(lambda: L.check(lib.mic_im2col(7, 1, 48, 16, P(px.t), P(out.t), out.ld, 0, None)), [out], "im2col dtype 7")
    # ViT assembly: S = 1, dtype
    x = can(4, 8)
    cls = vec(8, dev, "nan").put(np.ones((1, 8)))
    _refused(lambda: ops.vit_assemble(px.t, cls.t[0], cls.t, x.t, 4, 1, 8, 8), [x], "vit_assemble S 1")
    _refused(lambda: L.check(lib.mic_vit_assemble(7, 2, 2, 8, P(px.t), 8, P(cls.t), P(cls.t), P(x.t), None)), [x], "vit_assemble dtype 7")
    dcl, dps = vec(8, dev), can(2, 8, F32, off=4)
    _refused(lambda: L.check(lib.mic_vit_assemble_bwd(7, 2, 2, 8, P(px.t), P(x.t), 8, P(dcl.t), P(dps.t), None)), [x, dcl, dps], "vit_assemble_bwd dtype 7")
    _refused(lambda: ops.vit_assemble_bwd(px.t, x.t, dcl.t[0], dps.t, 2, 1, 8, 8), [x, dcl, dps], "vit_assemble_bwd S 1")
    # embeddings
    tab, ptab, h = ones(4, 16), ones(6, 16, F32), can(4, 16)
    _refused(lambda: ops.embed_fwd(i4, i4, tab.t, ptab.t, 1.0, h.t, 4, 12), [h], "embed_fwd width % 8")
    _refused(lambda: L.check(lib.mic_embed_fwd(7, 4, 16, P(i4), P(i4), P(tab.t), P(ptab.t), ctypes.c_float(1.0), P(h.t), None)), [h], "embed_fwd dtype 7")
    dtb, dpb = can(4, 16, F32, off=4), can(6, 16, F32, off=4)
    _refused(lambda: ops.embed_bwd(i4, i4, tab.t, 1.0, None, None, 4, 16), [dtb, dpb], "embed_bwd no output")
    _refused(lambda: ops.embed_bwd(None, i4, tab.t, 1.0, dtb.t, dpb.t, 4, 16), [dtb, dpb], "embed_bwd dtable without ids")
    _refused(lambda: L.check(lib.mic_embed_bwd(7, 4, 16, P(i4), P(i4), P(tab.t), ctypes.c_float(1.0), P(dtb.t), P(dpb.t), None)), [dtb, dpb], "embed_bwd dtype 7")
    # deterministic scatter: the table AND the workspace stay as found
    c = SC.DET_BY["det_13x1088"]
    ids, _ = SC.det_ids(c)
    dh, base = SC.det_inputs(c, "bf16")
    n, W, V = c["n"], c["width"], c["vocab"]
    dhb = mat(dh, BF, dev)
    big = ints(np.zeros(65540), dev)
    idd = big[:n]
    idd.copy_(torch.from_numpy(ids).to(dev))
    tb = Buf(V, W, W, F32, dev, "canary", off=4)
    ws = ops.embed_rows_add_det_workspace(V, dev)
    ws0 = ws.clone()
    det = lambda dtype=L.MIC_BF16, n=n, W=W, ids=idd, dh=dhb.t: L.check(lib.mic_embed_rows_add_det(  # noqa: E731
        dtype, n, W, V, P(ids), P(dh), ctypes.c_float(0.5), P(tb.t), P(ws), None))
    for what, call in (("dtype 7", lambda: det(dtype=7)), ("width % 64", lambda: det(W=1056)), ("n > 65536", lambda: det(n=65537, ids=big)),
                       ("misaligned ids", lambda: det(ids=big[1:])), ("misaligned dh", lambda: det(dh=dhb.full[:, 4:])),
                       ("n 0", lambda: det(n=0))):
        _refused(call, [tb], "embed_rows_add_det " + what)
        assert torch.equal(ws, ws0), f"embed_rows_add_det {what}: a refused call wrote to the workspace"
    tb.refill()
    tb.put(base)
    det()
    torch.cuda.synchronize()
    same_bits(tb.get(), SR.emu_det(ids, dh, 0.5, base).astype(np.float64), "a valid call after the refused ones")
    # column sums: a refused call has not zero-filled its output
    xb, o = ones(4, 16, pad=8), vec(16, dev)
    _refused(lambda: ops.colsum(xb.t, o.t[0], 4, 16, 20), [o], "colsum ld % 8")
    _refused(lambda: ops.colsum(xb.full[:4, 4:20], o.t[0], 4, 16, xb.ld), [o], "colsum x 8 B into a line")
    _refused(lambda: L.check(lib.mic_colsum(7, 4, 16, P(xb.t), xb.ld, P(o.t), 0, None)), [o], "colsum dtype 7")
    _refused(lambda: ops.colsum(xb.t, o.t[0], 0, 16, xb.ld), [o], "colsum rows 0")
    o2 = vec(16, dev)
    good = (xb.t, o.t[0], 4, 16, xb.ld)
    _refused(lambda: ops.colsum_grouped([good] * 8 + [(xb.t, o2.t[0], 4, 16, 20)]), [o, o2], "colsum_grouped: a bad ninth item")
    q = torch.zeros(4, 24, dtype=torch.uint8, device=dev).view(torch.float8_e5m2)
    sinv = torch.ones(1, device=dev)
    _refused(lambda: ops.colsum_q8_grouped([(q[:, :12], o.t[0], sinv, 4, 12)]), [o], "colsum_q8 cols % 8")
    _refused(lambda: ops.colsum_q8_grouped([(q[:, :16], o.t[0], sinv, 4, 16)] * 8 + [(q[:, :12], o2.t[0], sinv, 4, 12)]), [o, o2], "colsum_q8: a bad ninth item")
    item = L.ColsumQ8Item()
    item.x, item.out, item.scale_inv, item.rows, item.cols, item.ld, item.fmt = P(q), P(o.t), P(sinv), 4, 16, 24, 5
    _refused(lambda: L.check(lib.mic_colsum_q8_grouped(ctypes.byref(item), 1, None)), [o], "colsum_q8 fmt 5")
    # slabs: every condition
    src = torch.zeros(2 * 64 + 8, device=dev)
    d = can(4, 8, pad=8)
    ss = lambda **k: ops.sum_slabs(k.get("src", src), k.get("n", 2), k.get("stride", 64), k.get("dst", d.t), 4, k.get("cols", 8),  # noqa: E731
                                   k.get("lds", 12), k.get("ldd", d.ld))
    for what, kw in (("src misaligned", dict(src=src[1:])), ("dst misaligned", dict(dst=d.full[:4, 4:12])), ("n_slabs 0", dict(n=0)),
                     ("cols % 8", dict(cols=4)), ("ld_src % 4", dict(lds=10)), ("ld_dst % 8", dict(ldd=12)), ("slab_stride % 4", dict(stride=66))):
        _refused(lambda: ss(**kw), [d], "sum_slabs " + what)
    _refused(lambda: L.check(lib.mic_sum_slabs(7, 2, 64, 4, 8, P(src), 12, P(d.t), d.ld, None)), [d], "sum_slabs dtype 7")
    # row copies: 16-B rows
    s8, d8 = ones(4, 16, pad=8), can(4, 16, pad=8)
    _refused(lambda: ops.copy_rows(s8.t[:, :12], d8.t[:, :12], 4, 12), [d8], "copy_rows width % 8")
    _refused(lambda: L.check(lib.mic_copy_rows(L.MIC_BF16, 4, 16, P(s8.t), 20, None, P(d8.t), d8.ld, None, None)), [d8], "copy_rows ld_src % 8")
    _refused(lambda: L.check(lib.mic_copy_rows(L.MIC_BF16, 4, 16, P(s8.t), s8.ld, None, P(d8.t), 20, None, None)), [d8], "copy_rows ld_dst % 8")
    s4, d4 = ones(4, 8, F32), can(4, 8, F32)
    _refused(lambda: ops.copy_rows(s4.t[:, :6], d4.t[:, :6], 4, 6), [d4], "copy_rows fp32 width % 4")
    _refused(lambda: L.check(lib.mic_copy_rows(7, 4, 16, P(s8.t), s8.ld, None, P(d8.t), d8.ld, None, None)), [d8], "copy_rows dtype 7")
    # casts: a dtype pair the library does not know
    _refused(lambda: L.check(lib.mic_cast2d(7, L.MIC_BF16, 4, 16, P(s8.t), s8.ld, P(d8.t), d8.ld, None)), [d8], "cast2d src dtype 7")
    _refused(lambda: L.check(lib.mic_cast2d(L.MIC_F32, 7, 4, 8, P(s4.t), s4.ld, P(d8.t), d8.ld, None)), [d8], "cast2d dst dtype 7")
    _refused(lambda: L.check(lib.mic_cast(L.MIC_F32, 7, P(s4.t), P(d8.t), 8, None)), [d8], "cast dst dtype 7")
    _refused(lambda: ops.cast(s8.t, d8.t, 0), [d8], "cast n 0")
    # label terms: the ld conditions
    E, hh, dxs, dE = ones(4, 16, pad=8), ones(4, 16, pad=8), can(4, 16, F32, pad=4, off=4), can(4, 16, F32, off=4)
    cf = vec(4, dev, "nan").put(np.ones((1, 4)))
    hl = lambda **k: L.check(lib.mic_head_label_terms(4, k.get("W", 16), P(i4), P(cf.t), P(E.t), k.get("lde", E.ld), P(hh.t), k.get("ldh", hh.ld),  # noqa: E731
                                                      P(dxs.t), k.get("ldx", dxs.ld), P(dE.t), 16, None))
    for what, kw in (("width % 8", dict(W=12)), ("lde % 8", dict(lde=20)), ("ldh % 8", dict(ldh=20)), ("ldx % 4", dict(ldx=18))):
        _refused(lambda: hl(**kw), [dxs, dE], "head_label_terms " + what)
    # row flags: empty inputs; the dropout mask: p outside [0, 1)
    fl = Bytes(8, dev)
    for what, call in (("n_ids 0", lambda: L.check(lib.mic_row_flags(P(i4), 0, P(fl.t), 8, None))),
                       ("n_rows 0", lambda: L.check(lib.mic_row_flags(P(i4), 4, P(fl.t), 0, None))),
                       ("ids NULL", lambda: L.check(lib.mic_row_flags(None, 4, P(fl.t), 8, None))),
                       ("dropout p 1", lambda: L.check(lib.mic_dropout_mask(P(fl.t), 8, ctypes.c_float(1.0), 1, None)))):
        fl.refill()
        with pytest.raises(L.MicError):
            call()
        torch.cuda.synchronize()
        assert bool((fl.flat == 0xA5).all()), what
