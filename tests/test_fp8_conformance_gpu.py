"""fp8 emission conformance on the MI355X: every kernel that writes fp8 bytes, except the GEMM epilogues (the GEMM suite's fp8c_* cases),
against the reference of tests/util_fp8_ref.py — an encoder built from the OCP value tables alone and the emission contract
`emit_ref` / `emit_interval` — on the cases of tests/util_fp8_cases.py.

  quantiser   mic_fp8_amax, mic_fp8_quantize, mic_fp8_roll_amax: q, qT, state and the partial table equal emit_ref; every finite bf16
              bit pattern under current and delayed scaling; the tile edges, strides and pad tiles; grouped launches; block walks of
              the amax pass across item boundaries; a tile index beyond the partial table
  LayerNorm   mic_layernorm_fwd_q8, mic_layernorm_bwd_partials_q8: the bf16 tensors under the row-op suite's fp64 bounds, the bytes
              equal to emit_ref of the bf16 tensor as written; a run that drops the bf16 tensor gives the same bytes
  attention   mic_attn_bwd_q8 and cross-entropy mic_ce_bwd_q8 leave no bf16 copy: every byte lies in emit_interval of the fp64
              reference and its bound (util_attn_ref.bwd_ref, util_rowop_ref.ce_bwd_ref); the share of bytes that differ from the
              nominal Q(round(y)) is printed, not asserted
Around every call the outputs are windows in canary-filled allocations (0xA5 bytes, the NaN-payload canaries of the other suites):
rows behind `rows`, bytes between the columns and the row stride, rows of a packed batch that belong to no sequence keep their bits;
sources hold large finite values behind `rows` / `cols` (they must not reach the amax) or NaN where nothing may be read.

Kernels in scope (the committed listing profiles/fp8_conformance_kernel_stats.txt holds every one):
    fp8_amax_kernel  fp8_quantize_kernel  fp8_roll_kernel  ln_fwd_kernel<unsigned short, true>
    ln_bwd_kernel<unsigned short, {2,4}, 8, {1,2}>  attn_bwd_kernel<unsigned short, true>  ce_bwd_q8_kernel

Non-finite inputs are outside the checked domain.  What the code does with them: a NaN element is clamped away (fmaxf / fminf return
their other operand, so it leaves as the -FMAX byte) and does not enter the amax (fmaxf(m, NaN) = m); +-Inf saturates to +-FMAX and
makes the recorded amax infinite.  Nothing here asserts that."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_fp8_cases as FC  # noqa: E402
import util_fp8_ref as FR  # noqa: E402
import util_rowop_cases as RC  # noqa: E402
import util_rowop_ref as RR  # noqa: E402
from test_attn_conformance_gpu import Buf  # noqa: E402
from test_rowop_conformance_gpu import ints, put1, vec  # noqa: E402

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
TFMT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
CANARY8 = 0xA5


class Buf8:
    """a [rows][cols] window of bytes with row stride ld, 16 bytes into a 0xA5-filled allocation with `extra` rows and 16 bytes behind"""

    def __init__(self, rows, cols, ld, dev, extra=3, off=16):
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.flat = torch.empty(off + (rows + extra) * ld + 16, dtype=torch.uint8, device=dev)
        self.full = self.flat[off:off + (rows + extra) * ld].view(rows + extra, ld)
        self.t = self.full[:rows, :cols]
        self.refill()

    def refill(self):
        self.flat.fill_(CANARY8)
        return self

    def as_fmt(self, fmt, c0=0, n=None):
        return self.full[:self.rows, c0:c0 + (self.cols - c0 if n is None else n)].view(TFMT[fmt])

    def get(self):
        return self.t.cpu().numpy()

    def check_canary(self, what, written=None):
        """everything outside the window (with `written` [rows][cols] bool: outside its True part) kept the canary"""
        w = torch.zeros(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        win = w[self.off:self.off + self.full.numel()].view(self.full.shape)[:self.rows, :self.cols]
        win[...] = True if written is None else torch.as_tensor(written).to(w.device)
        n = int(((self.flat != CANARY8) & ~w).sum().item())
        assert n == 0, f"{what}: {n} byte(s) outside the output window changed"


def slot(amax_old, dev):
    """(state [2] in a canary vector with state[0] = amax_old, the partial table in a canary vector, zeroed)"""
    st, tb = vec(2, dev), vec(FR.PARTIALS, dev)
    put1(st, [amax_old, 0.0])
    tb.t.zero_()
    return st, tb


def f32np(b):
    return b.t[0].cpu().numpy()


def src_buf(full, rows, cols, dev):
    """a bf16 source: the numpy allocation [rows + extra][ld] copied whole (what lies behind rows / cols included), 16-B aligned"""
    t = torch.from_numpy(np.ascontiguousarray(full)).to(BF).to(dev)
    return t, t[:rows, :cols]


def _mic_err():
    from mic_amd._lib import MicError

    return MicError


# ------------------------------------------------------------------------------------------------ quantiser
@pytest.fixture(scope="module")
def exhaustive():
    return FC.all_finite_bf16()


@pytest.mark.parametrize("kind", list(FC.EXH_AMAX))
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_quantize_every_finite_bf16(dev, exhaustive, fmt, kind):
    from mic_amd import ops

    v = exhaustive
    a_old = FC.EXH_AMAX[kind]
    a_old = FC.tiny_amax(fmt) if a_old == "tiny" else a_old
    src = torch.from_numpy(v).to(BF).to(dev)
    assert np.array_equal(src.float().cpu().numpy().view(np.uint32), v.view(np.uint32)), "the source does not hold the bit patterns"
    q, qT = Buf8(256, 256, 256 + 8, dev), Buf8(256, 256, 256 + 16, dev)
    st, tb = slot(0.0 if a_old is None else a_old, dev)
    it = ops.fp8_item(src, 256, 256, st.t[0], TFMT[fmt], q=q.as_fmt(fmt), qT=qT.as_fmt(fmt), rows_pad=256,
                      amax_next=None if a_old is None else tb.t[0])
    ops.fp8_quantize([it], amax_pass=a_old is None)
    torch.cuda.synchronize()
    for o in (q, qT, st, tb):
        o.check_canary(f"exhaustive {fmt} {kind}")
    exp = FR.quant_expect(v, 256, 256, 256, fmt, a_old)
    got = dict(q=q.get(), qT=qT.get(), state=f32np(st), table=None if a_old is None else f32np(tb))
    FR.check_quant(exp, got, f"every finite bf16, {kind}", fmt)
    assert FR.is_finite_byte(got["q"], fmt).all(), "a NaN / Inf byte from finite inputs"
    assert not (got["q"][v == 0] & 0x7F).any(), "a zero input did not leave as a zero byte"
    if kind in ("saturating", "tiny"):
        assert ((got["q"] & 0x7F) == len(FR.GRID[fmt]) - 1).any()
    if kind == "top":
        sub = (got["q"] & 0x7F) < (8 if fmt == "e4m3" else 4)
        assert sub.mean() > 0.8, "the case does not reach the subnormal bytes"


@pytest.mark.parametrize("mode", FC.OUT_MODES)
@pytest.mark.parametrize("fmt", FR.FMTS)
@pytest.mark.parametrize("name", [g[0] for g in FC.GEOMETRY])
def test_quantize_geometry(dev, name, fmt, mode):
    """current scaling (amax pass) and delayed scaling on the same source; q only, qT only, both"""
    from mic_amd import ops

    _, rows, cols, rp, eld, eldq, eldqT = FC.GEOMETRY_BY[name]
    full = FC.geometry_source(name, fmt)
    alloc, _ = src_buf(full, rows, cols, dev)
    for a_old in (None, 4.0):
        q = Buf8(rows, cols, cols + eldq, dev) if mode != "qT" else None
        qT = Buf8(cols, rp, rp + eldqT, dev) if mode != "q" else None
        st, tb = slot(0.0 if a_old is None else a_old, dev)
        it = ops.fp8_item(alloc, rows, cols, st.t[0], TFMT[fmt], q=q.as_fmt(fmt) if q else None, qT=qT.as_fmt(fmt) if qT else None,
                          rows_pad=rp, amax_next=None if a_old is None else tb.t[0])
        assert it.ld == cols + eld
        ops.fp8_quantize([it], amax_pass=a_old is None)
        torch.cuda.synchronize()
        what = f"{name} {mode} {'current' if a_old is None else 'delayed'}"
        for o in (q, qT, st, tb):
            if o is not None:
                o.check_canary(what)
        exp = FR.quant_expect(full, rows, cols, rp, fmt, a_old)
        assert exp["amax"] == -FC.GEOMETRY_MAX, "the case's maximum is not the one placed in the last row and column"
        got = dict(q=q.get() if q else None, qT=qT.get() if qT else None, state=f32np(st), table=None if a_old is None else f32np(tb))
        FR.check_quant(exp, got, what, fmt)


def test_quantize_grouped_two_tables(dev):
    """ten items (two tables per launch) of mixed formats, shapes and output modes: once under current scaling (amax pass and
    quantiser, both grouped), once under delayed scaling with a table per item"""
    from mic_amd import ops

    for scaling in ("current", "delayed"):
        items, keep = [], []
        for i, (rows, cols, rp, fmt, mode, a_del) in enumerate(FC.GROUPED):
            a_old = None if scaling == "current" else a_del
            full = FC.grouped_source(i)
            alloc, _ = src_buf(full, rows, cols, dev)
            q = Buf8(rows, cols, cols + 8, dev) if mode != "qT" else None
            qT = Buf8(cols, rp, rp + 16, dev) if mode != "q" else None
            st, tb = slot(0.0 if a_old is None else a_old, dev)
            items.append(ops.fp8_item(alloc, rows, cols, st.t[0], TFMT[fmt], q=q.as_fmt(fmt) if q else None, qT=qT.as_fmt(fmt) if qT else None,
                                      rows_pad=rp, amax_next=None if a_old is None else tb.t[0]))
            keep.append((full, alloc, q, qT, st, tb, a_old))
        assert len(items) > 8
        ops.fp8_quantize(items, amax_pass=scaling == "current")
        torch.cuda.synchronize()
        for i, ((rows, cols, rp, fmt, mode, _), (full, _, q, qT, st, tb, a_old)) in enumerate(zip(FC.GROUPED, keep)):
            what = f"grouped item {i} {rows}x{cols} {mode} {scaling}"
            for o in (q, qT, st, tb):
                if o is not None:
                    o.check_canary(what)
            got = dict(q=q.get() if q else None, qT=qT.get() if qT else None, state=f32np(st), table=None if a_old is None else f32np(tb))
            FR.check_quant(FR.quant_expect(full, rows, cols, rp, fmt, a_old), got, what, fmt)


def test_amax_block_walks_cross_item_boundaries(dev):
    """eight items of 65 tiles: 520 tiles, two per block; every item's maximum in the tile next to an item boundary"""
    from mic_amd import _lib as L
    from mic_amd import ops

    n, rows, cols = FC.AMAX_WALK["items"], FC.AMAX_WALK["rows"], FC.AMAX_WALK["cols"]
    assert n * ((rows + 63) // 64) * ((cols + 63) // 64) > 512 and ((cols + 63) // 64) % 2 == 1
    items, keep = [], []
    for i in range(n):
        v = FC.amax_walk_source(i)
        src = torch.from_numpy(v).to(BF).to(dev)
        st = vec(2, dev)
        put1(st, [0.0, 0.0])
        q = Buf8(rows, cols, cols, dev)
        items.append(ops.fp8_item(src, rows, cols, st.t[0], TFMT["e4m3" if i % 2 else "e5m2"], q=q.as_fmt("e4m3" if i % 2 else "e5m2")))
        keep.append((v, src, st, q))
    arr = (L.Fp8Item * n)(*items)
    L.check(L.lib().mic_fp8_amax(arr, n, ops._stream()), "mic_fp8_amax")
    torch.cuda.synchronize()
    for i, (v, _, st, _) in enumerate(keep):
        st.check_canary(f"item {i}")
        got = f32np(st)
        assert got[0] == np.abs(v).max() == 20.0 + i and got[1] == 0.0, f"item {i}: amax {got[0]!r}, the tensor's is {np.abs(v).max()!r}"
    print(f"[conformance] amax/f32 state[0]: {n} items of 65 tiles, two tiles per block: equal")
    ops.fp8_quantize(items, amax_pass=False)   # and the quantiser on those scales
    torch.cuda.synchronize()
    for i, (v, _, st, q) in enumerate(keep):
        fmt = "e4m3" if i % 2 else "e5m2"
        FR.check_quant(FR.quant_expect(v, rows, cols, rows, fmt, None), dict(q=q.get(), state=f32np(st)), f"walk item {i}", fmt)


def test_partial_table_index_wraps(dev):
    """1025 quantiser tiles, the maximum in tile 1024: the table records it (slot 1024 & 1023 = 0)"""
    from mic_amd import ops

    rows, cols = FC.WRAP["rows"], FC.WRAP["cols"]
    assert (rows + 127) // 128 * ((cols + 63) // 64) > FR.PARTIALS
    v = FC.wrap_source()
    assert np.abs(v[:131072]).max() < np.abs(v[131072:]).max()
    src = torch.from_numpy(v).to(BF).to(dev)
    q = Buf8(rows, cols, cols, dev)
    st, tb = slot(6.0, dev)
    ops.fp8_quantize([ops.fp8_item(src, rows, cols, st.t[0], TFMT["e4m3"], q=q.as_fmt("e4m3"), amax_next=tb.t[0])], amax_pass=False)
    torch.cuda.synchronize()
    for o in (q, st, tb):
        o.check_canary("wrap")
    FR.check_quant(FR.quant_expect(v, rows, cols, rows, "e4m3", 6.0), dict(q=q.get(), state=f32np(st), table=f32np(tb)), "131200x64", "e4m3")


def test_roll_amax(dev):
    """five slots, stride 3: the table's maximum moves into state[slot][0], the tables are cleared, a slot with an all-zero table and
    every other entry of the state keep their bits"""
    from mic_amd import ops

    s0, p0 = FC.roll_inputs()
    st = Buf(5, 3, 3, F32, dev, "canary", off=4, extra=0)
    pt = Buf(5, FR.PARTIALS, FR.PARTIALS, F32, dev, "canary", off=4, extra=0)
    st.put(s0.astype(np.float64))
    pt.put(p0.astype(np.float64))
    ops.fp8_roll_amax(st.t, pt.t, 5)
    torch.cuda.synchronize()
    st.check_canary("roll state")
    pt.check_canary("roll partials")
    FR.check_roll(s0, p0, st.t.cpu().numpy(), pt.t.cpu().numpy(), "5 slots, stride 3")
    assert st.t[2, 0].item() == s0[2, 0] and st.t[4, 0].item() == np.float32(2e-30)


# ------------------------------------------------------------------------------------------------ LayerNorm forward
def _ln_fwd_run(dev, x, g, b, p, a_old, fmt, keep_y):
    from mic_amd import ops

    rows, W = x.shape
    xd = Buf(rows, W, W, BF, dev, "nan").put(x)
    gd, bd = put1(vec(W, dev, "nan"), g), put1(vec(W, dev, "nan"), b)
    y = Buf(rows, W, W, BF, dev, "canary") if keep_y else None
    mean, rstd = vec(rows, dev), vec(rows, dev)
    q = Buf8(rows, W, W + 8, dev)
    st, tb = slot(a_old, dev)
    ops.layernorm_fwd(xd.t, gd.t[0], bd.t[0], RC.LN_EPS, y.t if y else None, mean.t[0], rstd.t[0], rows=rows, dropout_p=p,
                      dropout_seed=FC.LN_SEED, q8=ops.fp8_out(q.as_fmt(fmt), st.t[0], tb.t[0]))
    torch.cuda.synchronize()
    for o in (y, mean, rstd, q, st, tb):
        if o is not None:
            o.check_canary(f"ln_fwd_q8 {rows}x{W}")
    assert f32np(st)[0] == np.float32(a_old), "state[0] moved"
    return dict(y=y.get() if y else None, mean=mean.get()[0], rstd=rstd.get()[0], q=q.get(), state1=f32np(st)[1], table=f32np(tb),
                stat_bits=(mean.bits(), rstd.bits()))


def _ln_fwd_both(dev, x, g, b, p, a_old, fmt, what):
    kept = _ln_fwd_run(dev, x, g, b, p, a_old, fmt, True)
    f = FR.check_ln_fwd_q8(x, g, b, RC.LN_EPS, p, FC.LN_SEED, a_old, fmt, kept, what)
    dropped = _ln_fwd_run(dev, x, g, b, p, a_old, fmt, False)
    FR.check_same_emission(dropped, kept, f"ln_fwd_q8/{fmt} y dropped: {what}")
    assert all(torch.equal(a, c) for a, c in zip(dropped["stat_bits"], kept["stat_bits"])), f"{what}: mean / rstd differ without y"
    return kept, f


@pytest.mark.parametrize("p", FC.LN_DROPOUT)
@pytest.mark.parametrize("rows,width", FC.LN_SHAPES)
def test_ln_fwd_q8(dev, rows, width, p):
    x, g, b, _, _ = RC.ln_inputs(FC.ln_case(rows, width), "bf16")
    keep = RR.keep_mask(x.size, p, FC.LN_SEED)
    a_old = float(np.float32(0.6 * np.abs(RR.ln_fwd_ref(x, g, b, RC.LN_EPS, "bf16", keep, p)["y"]).max()))   # the largest entries saturate
    kept, _ = _ln_fwd_both(dev, x, g, b, p, a_old, "e4m3", f"{rows}x{width} p={p}")
    assert ((kept["q"] & 0x7F) == 0x7E).any() and kept["table"].max() > a_old, "the case does not saturate"
    if p > 0:
        assert not (kept["q"].reshape(-1)[~RR.keep_mask(x.size, p, FC.LN_SEED)] & 0x7F).any(), "a dropped element is not a zero byte"


def test_ln_fwd_q8_wave_index_wraps(dev):
    """1030 rows (wave index = row): the tensor's maximum is in row 1027"""
    x, g, b = FC.ln_wrap_inputs()
    kept, f = _ln_fwd_both(dev, x, g, b, 0.0, 1.0, "e5m2", "1030x8, maximum in row 1027")
    assert np.abs(f["y"]).max(1).argmax() == 1027 and np.abs(f["y"][:1024]).max() < 0.8 * np.abs(f["y"][1027]).max()


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def _ln_bwd_run(dev, ops, xd, gd, mean, rstd, dyd, drd, rows, W, mode, p, a_old, fmt, keep_dxm):
    dx = Buf(rows, W, W, BF, dev, "canary")
    dxm = Buf(rows, W, W, BF, dev, "canary") if (mode == "dxm" and keep_dxm) else None
    nblk = ops.layernorm_bwd_blocks(rows)
    part = Buf(2 * nblk, W, W, F32, dev, "canary", off=4)
    q = Buf8(rows, W, W + 16, dev)
    st, tb = slot(a_old, dev)
    ops.layernorm_bwd_partials(xd.t, gd.t[0], mean.t[0], rstd.t[0], dyd.t, dx.t, part.t, rows=rows, dres=drd.t if drd else None,
                               dxm=dxm.t if dxm else None, dropout_p=p, dropout_seed=9, q8=ops.fp8_out(q.as_fmt(fmt), st.t[0], tb.t[0]),
                               q8_of_dx=mode == "dx")
    torch.cuda.synchronize()
    for o in (dx, dxm, part, q, st, tb):
        if o is not None:
            o.check_canary(f"ln_bwd_q8 {rows}x{W} {mode}")
    return dict(dx=dx.get(), dxm=dxm.get() if dxm else None, part=part.get().reshape(2, nblk, W), q=q.get(), state1=f32np(st)[1],
                table=f32np(tb), dx_bits=dx.bits())


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("mode,p", FC.LNB_MODES)
@pytest.mark.parametrize("rows,width", FC.LNB_SHAPES)
def test_ln_bwd_q8(dev, rows, width, mode, p, with_dres):
    from mic_amd import ops

    W = width
    x, g, b, dy, dres = RC.ln_inputs(FC.ln_case(rows, W), "bf16")
    xd, dyd = Buf(rows, W, W, BF, dev, "nan").put(x), Buf(rows, W, W, BF, dev, "nan").put(dy)
    drd = Buf(rows, W, W, BF, dev, "nan").put(dres) if with_dres else None
    gd, bd = put1(vec(W, dev, "nan"), g), put1(vec(W, dev, "nan"), b)
    mean, rstd = vec(rows, dev, "nan"), vec(rows, dev, "nan")
    ops.layernorm_fwd(xd.t, gd.t[0], bd.t[0], RC.LN_EPS, Buf(rows, W, W, BF, dev, "canary").t, mean.t[0], rstd.t[0], rows=rows)
    # the scale: 0.6 of the maximum of the fp64 gradient, so the largest entries saturate
    mu, rs = mean.get()[0], rstd.get()[0]
    a_old = float(np.float32(0.6 * np.abs(RR.ln_bwd_ref(x, g, mu, rs, dy, "bf16", dres=dres if with_dres else None)["dx"]).max()))
    what = f"{rows}x{W} {mode}{' dres' if with_dres else ''} p={p}"
    kept = _ln_bwd_run(dev, ops, xd, gd, mean, rstd, dyd, drd, rows, W, mode, p, a_old, "e5m2", True)
    FR.check_ln_bwd_q8(x, g, mu, rs, dy, dres if with_dres else None, p, 9, mode, a_old, "e5m2", kept, what)
    assert ((kept["q"] & 0x7F) == 0x7B).any(), "the case does not saturate"
    if mode == "dxm":
        dropped = _ln_bwd_run(dev, ops, xd, gd, mean, rstd, dyd, drd, rows, W, mode, p, a_old, "e5m2", False)
        FR.check_same_emission(dropped, kept, f"ln_bwd_q8/e5m2 dxm dropped: {what}")
        assert torch.equal(dropped["dx_bits"], kept["dx_bits"]) and np.array_equal(dropped["part"], kept["part"])


# ------------------------------------------------------------------------------------------------ attention backward
def _attn_run(dev, c, a_olds=None, fmt="e5m2"):
    """forward (bf16 out / lse as stored) and the fp8-emitting backward.  -> (refs, amax_olds, got)"""
    from mic_amd import ops

    q, k, v, do, km, q_off = FC.attn_inputs(c)
    B, H, Tq, Tk, HD = c["B"], c["H"], c["Tq"], c["Tk"], c["H"] * 64
    nq, nk = q.shape[0], k.shape[0]
    fused = c["layout"] == "fused3"
    if fused:
        ob = Buf(nq, 3 * HD, 3 * HD + 8, BF, dev, "nan").put(q).put(k, HD).put(v, 2 * HD)
        qd, kd, vd, ldq, ldk = ob.cols_of(0, HD), ob.cols_of(HD, HD), ob.cols_of(2 * HD, HD), ob.ld, ob.ld
    else:
        qb = Buf(nq, HD, HD + 8, BF, dev, "nan").put(q)
        kb = Buf(nk, 2 * HD, 2 * HD + 16, BF, dev, "nan").put(k).put(v, HD)
        qd, kd, vd, ldq, ldk = qb.t, kb.cols_of(0, HD), kb.cols_of(HD, HD), qb.ld, kb.ld
    dod = Buf(nq, HD, HD + 16, BF, dev, "nan").put(do)
    out = Buf(nq, HD, HD + 8, BF, dev, "canary")
    lse = Buf(1, B * H * Tq, B * H * Tq, F32, dev, "canary", off=4, extra=0)
    kmd = torch.from_numpy(km).to(dev) if km is not None else None
    offd = torch.from_numpy(q_off).to(dev) if q_off is not None else None
    lend = torch.tensor(c["q_len"], dtype=torch.int32, device=dev) if q_off is not None else None
    if q_off is not None:
        ops.attn_fwd_packed(qd, kd, vd, out.t, B, H, Tq, Tk, offd, lend, kv_packed=c["kv_packed"], ldq=ldq, ldk=ldk, ldv=ldk, ldo=out.ld,
                            causal=c["causal"], lse=lse.t)
    else:
        ops.attn_fwd(qd, kd, vd, out.t, B, H, Tq, Tk, ldq=ldq, ldk=ldk, ldv=ldk, ldo=out.ld, key_mask=kmd, causal=c["causal"], lse=lse.t)
    torch.cuda.synchronize()
    o_st = np.nan_to_num(out.get())                      # rows of no sequence hold the canary: never read by the reference
    l_st = np.nan_to_num(lse.get().reshape(B, H, Tq), nan=0.0, neginf=-np.inf)
    refs = FR.attn_q8_ref(c, q, k, v, do, km, q_off, o_st, l_st)
    a_olds = FR.attn_amax_old(refs) if a_olds is None else a_olds
    slots = [slot(a, dev) for a in a_olds]
    if fused:
        bufs = [Buf8(nq, 3 * HD, 3 * HD + 8, dev)]
        qb8 = bufs[0]
        dq8, dk8, dv8 = (ops.fp8_out(qb8.as_fmt(fmt), slots[0][0].t[0], slots[0][1].t[0]),
                         ops.fp8_out(qb8.as_fmt(fmt, HD), slots[0][0].t[0], slots[0][1].t[0]), qb8.as_fmt(fmt, 2 * HD))
    else:
        bufs = [Buf8(nq, HD, HD + 8, dev), Buf8(nk, 2 * HD, 2 * HD + 16, dev)]
        dq8, dk8, dv8 = (ops.fp8_out(bufs[0].as_fmt(fmt), slots[0][0].t[0], slots[0][1].t[0]),
                         ops.fp8_out(bufs[1].as_fmt(fmt), slots[1][0].t[0], slots[1][1].t[0]), bufs[1].as_fmt(fmt, HD))
    ops.attn_bwd_q8(qd, kd, vd, out.t, dod.t, lse.t, dq8, dk8, dv8, B, H, Tq, Tk, ldq=ldq, ldk=ldk, ldv=ldk, ldo=out.ld, lddo=dod.ld,
                    q_off=offd, q_len=lend, kv_packed=c["kv_packed"], key_mask=kmd, causal=c["causal"])
    torch.cuda.synchronize()
    got = []
    for (name, y, e, w), b8, (st, tb) in zip(refs, bufs, slots):
        b8.check_canary(f"{c['name']} {name}: rows of no sequence, bytes behind the head columns",
                        np.repeat(w[:, None], b8.cols, 1))
        st.check_canary(name)
        tb.check_canary(name)
        got.append((b8.get(), f32np(st)[1], f32np(tb)))
    return refs, a_olds, got


@pytest.mark.parametrize("name", [c["name"] for c in FC.ATTN])
def test_attn_bwd_q8(dev, name):
    c = FC.ATTN_BY[name]
    refs, a_olds, got = _attn_run(dev, c)
    FR.check_attn_q8(refs, a_olds, "e5m2", got, name)
    assert len(refs) == (1 if c["layout"] == "fused3" else 2)


# ------------------------------------------------------------------------------------------------ CE backward
@pytest.mark.parametrize("V,Vpad", FC.CE_V)
@pytest.mark.parametrize("rows", FC.CE_ROWS)
def test_ce_bwd_q8(dev, rows, V, Vpad):
    from mic_amd import ops

    x, labels, mask, lse, denom = FC.ce_inputs(rows, V, Vpad)
    ld = Vpad + 8
    lg = Buf(rows, Vpad, ld, BF, dev, "nan").put(x)
    before = lg.bits()
    ld_, md = ints(labels, dev), ints(mask, dev)
    lsed, dend = put1(vec(rows, dev, "nan"), lse), put1(vec(1, dev, "nan"), [denom])
    start = np.linspace(-1, 1, Vpad).astype(np.float32).astype(np.float64) * 1e-3
    for fmt in FR.FMTS:
        for ls in FC.CE_LS:
            what = f"{rows}x{V}/{Vpad}"
            plain = None
            for with_coef in (False, True):
                q, st, cs = Buf8(rows, Vpad, Vpad + 8, dev), vec(2, dev), put1(vec(Vpad, dev), start)
                coef = vec(rows, dev) if with_coef else None
                ops.ce_bwd_q8(lg.t, ld, V, Vpad, ld_, md, ls, lsed.t[0], dend.t[0], rows, ops.fp8_out(q.as_fmt(fmt), st.t[0]), colsum=cs.t[0],
                              label_coef=coef.t[0] if coef else None, loss_scale=FC.CE_LOSS_SCALE)
                torch.cuda.synchronize()
                for o in (q, st, cs, coef):
                    if o is not None:
                        o.check_canary(what)
                assert torch.equal(lg.bits(), before), f"{what}: the logits changed"
                got = dict(q=q.get(), state=f32np(st), coef=f32np(coef) if coef else None, colsum=f32np(cs))
                FR.check_ce_q8(x, V, labels, mask, ls, lse, denom, FC.CE_LOSS_SCALE, fmt, got, what + (" label_coef" if with_coef else ""),
                               colsum0=start, plain=plain)
                plain = got["q"]


# ------------------------------------------------------------------------------------------------ tiny amax
@pytest.mark.parametrize("fmt", FR.FMTS)
@pytest.mark.parametrize("family", ["ln_fwd", "ln_bwd", "attn_bwd"])
def test_tiny_amax_keeps_zeros_and_finite_bytes(dev, family, fmt):
    """amax_old just below FMAX / FLT_MAX (FMAX / amax_old overflows) and a tensor that contains zeros: zero inputs leave as zero bytes,
    no byte is NaN / Inf, and the bytes are emit_ref's (scale clamped at FLT_MAX: every non-zero element saturates).  The quantiser's
    case is test_quantize_every_finite_bf16[tiny]."""
    from mic_amd import ops

    a_old = FC.tiny_amax(fmt)
    assert not np.isfinite(np.float32(FR.FMAX[fmt]) / np.float32(a_old)) and a_old > 1.1754944e-38
    if family == "ln_fwd":
        x, g, b, _, _ = RC.ln_inputs(FC.ln_case(7, 72), "bf16")
        kept = _ln_fwd_run(dev, x, g, b, 0.1, a_old, fmt, True)
        FR.check_emitted(kept["y"], a_old, fmt, kept, f"tiny amax ln_fwd_q8/{fmt}")
        src, q = kept["y"], kept["q"]
    elif family == "ln_bwd":
        rows, W = 9, 72
        x, g, b, dy, _ = RC.ln_inputs(FC.ln_case(rows, W), "bf16")
        xd, dyd = Buf(rows, W, W, BF, dev, "nan").put(x), Buf(rows, W, W, BF, dev, "nan").put(dy)
        gd, bd = put1(vec(W, dev, "nan"), g), put1(vec(W, dev, "nan"), b)
        mean, rstd = vec(rows, dev, "nan"), vec(rows, dev, "nan")
        ops.layernorm_fwd(xd.t, gd.t[0], bd.t[0], RC.LN_EPS, Buf(rows, W, W, BF, dev, "canary").t, mean.t[0], rstd.t[0], rows=rows)
        kept = _ln_bwd_run(dev, ops, xd, gd, mean, rstd, dyd, None, rows, W, "dxm", 0.1, a_old, fmt, True)
        FR.check_emitted(kept["dxm"], a_old, fmt, kept, f"tiny amax ln_bwd_q8/{fmt}")
        src, q = kept["dxm"], kept["q"]
    else:
        c = FC.ATTN_BY["aq_self_64_causal_masked_tail"]
        refs, a_olds, got = _attn_run(dev, c, a_olds=[a_old], fmt=fmt)
        FR.check_attn_q8(refs, a_olds, fmt, got, f"tiny amax {c['name']}")
        (_, y, e, w), q = refs[0], got[0][0][refs[0][3]]
        src = np.where((y[w] == 0) & (e[w] == 0), 0.0, 1.0)   # exact zeros of the reference: the gradients of masked keys
    assert (src == 0).any() and (src != 0).any(), "the case holds no zeros"
    assert FR.is_finite_byte(q, fmt).all(), "a NaN / Inf byte from finite inputs"
    assert not (q[src == 0] & 0x7F).any(), "a zero input did not leave as a zero byte"


# ------------------------------------------------------------------------------------------------ refusals
def _refused8(fn, outs, what):
    """MicError on the host, before any launch: every output keeps its canary"""
    for o in outs:
        o.refill()
    with pytest.raises(_mic_err()):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        o.check_canary(what, torch.zeros(o.rows, o.cols, dtype=torch.bool))


def test_fp8_refusals(dev):
    """every MIC_CHECK condition of mic_fp8_amax, mic_fp8_quantize, mic_fp8_roll_amax, q8_check (through both LayerNorm entry points),
    mic_attn_bwd_q8 and mic_ce_bwd_q8: an error on the host, nothing written"""
    from mic_amd import _lib as L
    from mic_amd import ops

    E4 = TFMT["e4m3"]
    rows, cols = 32, 64
    src = torch.ones((rows + 1, cols + 8), dtype=BF, device=dev)
    st, tb = vec(2, dev), vec(FR.PARTIALS, dev)
    q, qT = Buf8(rows, cols, cols + 8, dev), Buf8(cols, rows, rows + 16, dev)
    outs = [q, qT, st, tb]

    def item(**kw):
        """a valid item with the named struct fields replaced (pointers as integers or None)"""
        it = ops.fp8_item(src, rows, cols, st.t[0], E4, q=q.as_fmt("e4m3"), qT=qT.as_fmt("e4m3"), rows_pad=rows, amax_next=tb.t[0])
        for k, v in kw.items():
            setattr(it, k, v)
        return it

    def both(what, **kw):
        for amax_pass in (True, False):
            _refused8(lambda: ops.fp8_quantize([item(**kw)], amax_pass=amax_pass), outs, f"{what} ({'amax' if amax_pass else 'quantize'})")

    for fn in ("mic_fp8_amax", "mic_fp8_quantize"):
        _refused8(lambda: L.check(getattr(L.lib(), fn)(None, 1, None), fn), outs, f"{fn} items NULL")
        _refused8(lambda: L.check(getattr(L.lib(), fn)((L.Fp8Item * 1)(item()), 0, None), fn), outs, f"{fn} count 0")
    both("src NULL", src=None)
    both("state NULL", state=None)
    both("rows 0", rows=0)
    both("cols 0", cols=0)
    both("ld < cols", ld=cols - 8)
    both("cols % 8", cols=60)
    both("ld % 8", ld=cols + 4)
    both("src 8 B into a 16-B line", src=src[:, 4:].data_ptr())
    both("format 7", fmt=7)
    qz = lambda **kw: _refused8(lambda: ops.fp8_quantize([item(**kw)], amax_pass=False), outs, f"quantize {sorted(kw)}")  # noqa: E731
    qz(q=None, qT=None)
    qz(ldq=cols - 8)
    qz(ldq=cols + 4)
    qz(q=q.full[:rows, 4:].data_ptr())
    qz(rows_pad=rows + 8, ldqT=rows + 24)
    qz(ldqT=rows - 16)
    qz(ldqT=rows + 8)
    qz(qT=qT.full[:cols, 8:].data_ptr())
    # roll
    s5, p5 = Buf(2, 3, 3, F32, dev, "canary", off=4, extra=0), Buf(2, FR.PARTIALS, FR.PARTIALS, F32, dev, "canary", off=4, extra=0)
    roll = lambda s, stride, p, n: L.check(L.lib().mic_fp8_roll_amax(s, stride, p, n, None), "roll")  # noqa: E731
    for what, args in (("state NULL", (None, 3, p5.t.data_ptr(), 2)), ("partials NULL", (s5.t.data_ptr(), 3, None, 2)),
                       ("stride 0", (s5.t.data_ptr(), 0, p5.t.data_ptr(), 2)), ("count 0", (s5.t.data_ptr(), 3, p5.t.data_ptr(), 0))):
        _refused8(lambda: roll(*args), [s5, p5], f"roll {what}")
    # q8_check through the LayerNorm entry points
    R, W = 4, 64
    x, dy = Buf(R, W, W, BF, dev, "nan").put(np.ones((R, W))), Buf(R, W, W, BF, dev, "nan").put(np.ones((R, W)))
    g = put1(vec(W, dev, "nan"), np.ones(W))
    stat = put1(vec(R, dev, "nan"), np.ones(R))
    y, dx, mean, rstd = Buf(R, W, W, BF, dev, "canary"), Buf(R, W, W, BF, dev, "canary"), vec(R, dev), vec(R, dev)
    part = Buf(2, W, W, F32, dev, "canary", off=4)
    q8 = Buf8(R, W, W + 8, dev)

    def out8(**kw):
        o = ops.fp8_out(q8.as_fmt("e5m2"), st.t[0], tb.t[0])
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    lnf = lambda o: ops.layernorm_fwd(x.t, g.t[0], g.t[0], 1e-5, y.t, mean.t[0], rstd.t[0], rows=R, q8=o)  # noqa: E731
    lnb = lambda o, p=part: ops.layernorm_bwd_partials(x.t, g.t[0], stat.t[0], stat.t[0], dy.t, dx.t, p.t if p else None, rows=R, q8=o)  # noqa: E731
    for what, kw in (("q NULL", dict(q=None)), ("state NULL", dict(state=None)), ("ldq < width", dict(ldq=W - 8)), ("ldq % 8", dict(ldq=W + 4)),
                     ("q 4 B into an 8-B word", dict(q=q8.full[:R, 4:].data_ptr())), ("format 7", dict(fmt=7))):
        _refused8(lambda: lnf(out8(**kw)), [y, mean, rstd, q8, st, tb], f"ln_fwd_q8 {what}")
        _refused8(lambda: lnb(out8(**kw)), [dx, part, q8, st, tb], f"ln_bwd_partials_q8 {what}")
    _refused8(lambda: lnb(out8(), None), [dx, q8, st, tb], "ln_bwd_partials_q8 partials NULL")
    null8 = lambda fn, *a: L.check(getattr(L.lib(), fn)(*a), fn)  # noqa: E731
    _refused8(lambda: null8("mic_layernorm_fwd_q8", R, W, x.t.data_ptr(), g.t.data_ptr(), g.t.data_ptr(), 1e-5, y.t.data_ptr(), None, None, 0.0, 0,
                            None, None), [y, q8], "ln_fwd_q8 q8 NULL")
    # attention
    B, H, T, HD = 2, 2, 64, 128
    mk = lambda fill: Buf(B * T, HD, HD + 8, BF, dev, fill)  # noqa: E731
    aq, ak, av, ao, ado = (mk("nan").put(np.ones((B * T, HD))) for _ in range(5))
    lse = put1(vec(B * H * T, dev, "nan"), np.zeros(B * H * T))
    dq8, dkv8 = Buf8(B * T, HD, HD + 8, dev), Buf8(B * T, 2 * HD, 2 * HD + 8, dev)
    s2, t2 = vec(2, dev), vec(FR.PARTIALS, dev)
    qo, ql = torch.tensor([0, 64], dtype=torch.int32, device=dev), torch.tensor([64, 64], dtype=torch.int32, device=dev)
    aouts = [dq8, dkv8, st, tb, s2, t2]

    def attn(**kw):
        oq = ops.fp8_out(dq8.as_fmt(kw.get("fq", "e5m2")), st.t[0], tb.t[0])
        ok = ops.fp8_out(dkv8.as_fmt(kw.get("fk", "e5m2")), s2.t[0], t2.t[0])
        for o, pre in ((oq, "q_"), (ok, "k_")):
            for f in ("q", "state", "fmt"):
                if pre + f in kw:
                    setattr(o, f, kw[pre + f])
        ld = dict(ldq=aq.ld, ldk=ak.ld, ldv=av.ld, ldo=ao.ld, lddo=ado.ld)
        ld.update({k: v for k, v in kw.items() if k in ld})
        ops.attn_bwd_q8(kw.get("q", aq.t), ak.t, av.t, ao.t, ado.t, kw.get("lse", lse.t[0]), oq, ok, kw.get("dv8", dkv8.as_fmt("e5m2", HD)), B, H,
                        kw.get("Tq", T), kw.get("Tk", T), q_off=kw.get("q_off"), q_len=kw.get("q_len"), **ld)

    for what, kw in (("dv8 NULL", dict(dv8=None)), ("q_off without q_len", dict(q_off=qo)), ("q_len without q_off", dict(q_len=ql)),
                     ("dq8.q NULL", dict(q_q=None)), ("dq8.state NULL", dict(q_state=None)), ("dk8.q NULL", dict(k_q=None)),
                     ("dk8.state NULL", dict(k_state=None)), ("formats differ", dict(fk="e4m3")), ("format 7", dict(q_fmt=7, k_fmt=7)),
                     ("Tq 65", dict(Tq=65)), ("Tk 65", dict(Tk=65)), ("q NULL", dict(q=None)), ("lse NULL", dict(lse=None)),
                     ("ldq % 8", dict(ldq=HD + 4)), ("lddo % 8", dict(lddo=HD + 4))):
        _refused8(lambda: attn(**kw), aouts, f"attn_bwd_q8 {what}")
    # cross-entropy
    rows, V, Vpad, ld = 4, 40, 40, 48
    lg = Buf(rows, Vpad, ld, BF, dev, "nan").put(np.zeros((rows, Vpad)))
    lab, msk = ints(np.zeros(rows), dev), ints(np.ones(rows), dev)
    lsev, den = put1(vec(rows, dev, "nan"), np.ones(rows)), put1(vec(1, dev, "nan"), [4.0])
    cq, cs, coef = Buf8(rows, Vpad, Vpad + 8, dev), vec(Vpad, dev), vec(rows, dev)
    couts = [cq, st, cs, coef]

    def ce(**kw):
        o = ops.fp8_out(cq.as_fmt("e5m2"), st.t[0])
        for f in ("q", "state", "ldq", "fmt"):
            if f in kw:
                setattr(o, f, kw[f])
        ops.ce_bwd_q8(kw.get("lg", lg.t), kw.get("ld", ld), kw.get("V", V), kw.get("Vpad", Vpad), kw.get("lab", lab), kw.get("msk", msk), 0.0,
                      kw.get("lse", lsev.t[0]), kw.get("den", den.t[0]), kw.get("rows", rows), o, colsum=cs.t[0], label_coef=coef.t[0])

    for what, kw in (("rows 0", dict(rows=0)), ("V 1", dict(V=1)), ("Vpad < V", dict(V=48, Vpad=40)), ("Vpad % 8", dict(V=37, Vpad=37)),
                     ("ld < Vpad", dict(ld=32)), ("ld % 8", dict(ld=44)), ("logits NULL", dict(lg=None)), ("labels NULL", dict(lab=None)),
                     ("mask NULL", dict(msk=None)), ("row_lse NULL", dict(lse=None)), ("denom NULL", dict(den=None)), ("q NULL", dict(q=None)),
                     ("state NULL", dict(state=None)), ("ldq < Vpad", dict(ldq=32)), ("ldq % 8", dict(ldq=44)),
                     ("q 4 B into an 8-B word", dict(q=cq.full[:rows, 4:].data_ptr())),
                     ("logits 8 B into a 16-B line", dict(lg=lg.full[:rows, 4:4 + Vpad])), ("format 7", dict(fmt=7))):
        _refused8(lambda: ce(**kw), couts, f"ce_bwd_q8 {what}")
    _refused8(lambda: null8("mic_ce_bwd_q8", rows, V, Vpad, lg.t.data_ptr(), ld, lab.data_ptr(), msk.data_ptr(), 0.0, lsev.t.data_ptr(),
                            den.t.data_ptr(), 1.0, None, None, None, None), couts, "ce_bwd_q8 q8 NULL")
