"""Row-op conformance on the MI355X: the LayerNorm family (csrc/norm.hip), the materialised-logits cross-entropy family
(csrc/elementwise.hip) and AdamW (csrc/optimizer.hip) on every case of tests/util_rowop_cases.py, in bf16 and fp32 where the entry point takes a dtype, against
the fp64 references and derived per-element bounds of tests/util_rowop_ref.py.  Around every call:
  - outputs are windows in canary-filled allocations (extra rows, a row stride wider than the columns where the entry point takes
    one, a base offset that keeps the documented alignment); every element outside the window keeps its bits;
  - what a kernel must not read holds NaN: operand rows past `rows`, columns V .. ld of the logits of mic_ce_rows /
    mic_ce_rows_tiles, stat entries past ntiles.  Columns V .. Vpad of mic_ce_bwd* are read as part of a chunk and discarded: they
    hold NaN too and must come back as zeros;
  - every path without atomics runs twice from the same inputs and gives identical bits (all but dgamma / dbeta of
    mic_layernorm_bwd and the colsum of mic_ce_bwd_t); in-place kernels get their inputs restored between the runs.
The backward of LayerNorm is checked on the mean / rstd it is handed (the device forward's, as stored) and once end to end.
Out of scope: the _q8 forms (tests/test_fp8_conformance_gpu.py checks their bf16 outputs against these references and their bytes
against an fp8 reference of its own); the decode epilogues are in tests/test_decode_conformance_gpu.py, embeddings, the ViT assembly and colsum in
tests/test_scatter_conformance_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_rowop_cases as RC  # noqa: E402
import util_rowop_ref as RR  # noqa: E402
from test_attn_conformance_gpu import IB, TD, Buf, _refused  # noqa: E402
from util_gemm_ref import U32, check, gamma_k, round_to  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32


def vec(n, dev, fill="canary", dtype=F32):
    """a 1-D window of n elements, 16 B into its allocation"""
    return Buf(1, n, n, dtype, dev, fill, off=4 if dtype == F32 else 8, extra=0)


def put1(b, x):
    return b.put(np.asarray(x, np.float64).reshape(1, -1))


def ints(x, dev, dtype=torch.int32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev)


def twice(run, outs, what, prep=None, inexact=()):
    """run the launch twice, each time from canary-refilled outputs (`prep` restores what an in-place kernel overwrote or zeroes an
    accumulator): identical bits, except for the outputs fed by atomics (`inexact`)"""
    first = None
    for _ in range(2):
        for o in outs:
            o.refill()
        if prep:
            prep()
        run()
        torch.cuda.synchronize()
        if first is None:
            first = [o.bits() for o in outs]
    for o, f in zip(outs, first):
        if not any(o is i for i in inexact):
            assert torch.equal(o.bits(), f), f"{what}: two runs differ"


def bits16(b):
    """the window of a bf16 Buf as uint16 numpy bits"""
    return b.t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def zero_bits(t):
    return not bool(t.contiguous().view(IB[t.dtype]).any().item())


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("p", RC.LN_DROPOUT)
@pytest.mark.parametrize("name", [c["name"] for c in RC.LN_FWD])
def test_ln_fwd(dev, name, p, dtype):
    from mic_amd import ops

    c, dt = RC.LN_ALL[name], TD[dtype]
    rows, W = c["rows"], c["width"]
    x, g, b, _, _ = RC.ln_inputs(c, dtype)
    xd = Buf(rows, W, W, dt, dev, "nan").put(x)
    gd, bd = put1(vec(W, dev, "nan"), g), put1(vec(W, dev, "nan"), b)
    y = Buf(rows, W, W, dt, dev, "canary")
    stats = [] if c.get("nostats") else [vec(rows, dev), vec(rows, dev)]
    twice(lambda: ops.layernorm_fwd(xd.t, gd.t[0], bd.t[0], RC.LN_EPS, y.t, *(s.t[0] for s in stats), rows=rows, dropout_p=p, dropout_seed=77),
          [y] + stats, name)
    for o in [y] + stats:
        o.check_canary(name)
    keep = RR.keep_mask(x.size, p, 77)
    if p > 0:
        assert np.array_equal(ops.dropout_mask(x.size, p, 77, dev).cpu().numpy().astype(bool), keep), "mic_dropout_mask"
    f = RR.ln_fwd_ref(x, g, b, RC.LN_EPS, dtype, keep, p)
    if stats:
        check(stats[0].get()[0], f["mean"], f["bound_mean"], f"ln_fwd/{dtype} mean: {name}")
        check(stats[1].get()[0], f["rstd"], f["bound_rstd"], f"ln_fwd/{dtype} rstd: {name}")
    check(y.get(), f["y"], f["bound_y"], f"ln_fwd/{dtype} y: {name}")
    if p > 0:
        assert zero_bits(y.t.reshape(-1)[torch.from_numpy(~keep).to(dev)]), f"{name}: a dropped element is not an exact zero"


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in RC.LN_BWD])
def test_ln_bwd(dev, name, dtype):
    from mic_amd import ops

    c, dt = RC.LN_ALL[name], TD[dtype]
    rows, W, fl = c["rows"], c["width"], RC.LN_FLAGS[c["flags"]]
    x, g, b, dy, dres = RC.ln_inputs(c, dtype)
    xd, dyd = Buf(rows, W, W, dt, dev, "nan").put(x), Buf(rows, W, W, dt, dev, "nan").put(dy)
    drd = Buf(rows, W, W, dt, dev, "nan").put(dres) if "dres" in fl else None
    gd, bd = put1(vec(W, dev, "nan"), g), put1(vec(W, dev, "nan"), b)
    ytmp = Buf(rows, W, W, dt, dev, "canary")
    mean, rstd = vec(rows, dev, "nan"), vec(rows, dev, "nan")
    ops.layernorm_fwd(xd.t, gd.t[0], bd.t[0], RC.LN_EPS, ytmp.t, mean.t[0], rstd.t[0], rows=rows)
    dx = Buf(rows, W, W, dt, dev, "canary")
    dxm = Buf(rows, W, W, dt, dev, "canary") if "dxm" in fl else None
    dg, db = vec(W, dev), (None if c.get("nobeta") else vec(W, dev))
    kw = dict(rows=rows, dres=drd.t if drd else None, dxm=dxm.t if dxm else None, dropout_p=0.1 if dxm else 0.0, dropout_seed=9,
              in_dropout_p=0.1 if "in_dropout" in fl else 0.0, in_dropout_seed=5)
    outs = [o for o in (dx, dxm, dg, db) if o is not None]
    acc = [o for o in (dg, db) if o is not None]
    twice(lambda: ops.layernorm_bwd(xd.t, gd.t[0], mean.t[0], rstd.t[0], dyd.t, dx.t, dg.t[0], db.t[0] if db else None, **kw), outs, name,
          prep=lambda: [a.t.zero_() for a in acc], inexact=acc)
    for o in outs:
        o.check_canary(name)
    mu, rs = mean.get()[0], rstd.get()[0]
    kin = RR.keep_mask(x.size, 0.1, 5) if "in_dropout" in fl else None
    dr = dres if drd else None
    r = RR.ln_bwd_ref(x, g, mu, rs, dy, dtype, dres=dr, keep_in=kin, p_in=0.1)
    check(dx.get(), r["dx"], r["bound_dx"], f"ln_bwd/{dtype} dx: {name}")
    check(dg.get()[0], r["dgamma"], r["bound_dgamma"], f"ln_bwd/{dtype} dgamma: {name}")
    if db:
        check(db.get()[0], r["dbeta"], r["bound_dbeta"], f"ln_bwd/{dtype} dbeta: {name}")
    if dxm:
        v, e = RR.dxm_ref(dx.get(), RR.keep_mask(x.size, 0.1, 9), 0.1, dtype)
        check(dxm.get(), v, e, f"ln_bwd/{dtype} dxm: {name}")
        assert zero_bits(dxm.t.reshape(-1)[torch.from_numpy(~RR.keep_mask(x.size, 0.1, 9)).to(dev)])
    if rows <= 50:  # once end to end: the statistics of the fp64 forward, the bound widened by the forward's bounds
        f = RR.ln_fwd_ref(x, g, b, RC.LN_EPS, dtype)
        e = RR.ln_bwd_ref(x, g, f["mean"], f["rstd"], dy, dtype, dres=dr, keep_in=kin, p_in=0.1, fwd=f)
        check(dx.get(), e["dx"], e["bound_dx"], f"ln_bwd/{dtype} dx end to end: {name}")
        check(dg.get()[0], e["dgamma"], e["bound_dgamma"], f"ln_bwd/{dtype} dgamma end to end: {name}")
    # the partials form: the same dx / dxm bits, partials [2][blocks][width] fully overwritten inside a canary, their sums within the
    # bounds of dgamma / dbeta, mic_ln_param_grads overwriting (accumulate 0) and adding to a start vector (accumulate 1)
    nblk = ops.layernorm_bwd_blocks(rows)
    assert nblk == RC.ln_bwd_blocks(rows)
    part = Buf(2 * nblk, W, W, F32, dev, "canary", off=4)
    dx2 = Buf(rows, W, W, dt, dev, "canary")
    dxm2 = Buf(rows, W, W, dt, dev, "canary") if dxm else None
    kw2 = dict(kw, dxm=dxm2.t if dxm2 else None)
    twice(lambda: ops.layernorm_bwd_partials(xd.t, gd.t[0], mean.t[0], rstd.t[0], dyd.t, dx2.t, part.t, **kw2), [o for o in (dx2, dxm2, part) if o], name)
    part.check_canary(name + " partials")
    assert torch.equal(dx2.bits(), dx.bits()) and (dxm is None or torch.equal(dxm2.bits(), dxm.bits())), f"{name}: partials form, other dx bits"
    P = part.get().reshape(2, nblk, W)
    assert np.isfinite(P).all(), f"{name}: an entry of the partials was not written"
    check(P[0].sum(0), r["dgamma"], r["bound_dgamma"], f"ln_bwd/{dtype} partials dgamma: {name}")
    check(P[1].sum(0), r["dbeta"], r["bound_dbeta"], f"ln_bwd/{dtype} partials dbeta: {name}")
    og, ob = vec(W, dev), vec(W, dev)
    twice(lambda: ops.ln_param_grads([(part.t, nblk, W, og.t[0], ob.t[0], False)]), [og, ob], name + " param_grads")
    bnd = lambda k: gamma_k(nblk) * np.abs(P[k]).sum(0) + 1e-300  # noqa: E731
    check(og.get()[0], P[0].sum(0), bnd(0), f"ln_param_grads/f32 dgamma: {name}")
    check(ob.get()[0], P[1].sum(0), bnd(1), f"ln_param_grads/f32 dbeta: {name}")
    start = np.linspace(-1, 1, W).astype(np.float32).astype(np.float64)
    twice(lambda: ops.ln_param_grads([(part.t, nblk, W, og.t[0], None, True)]), [og, ob], name + " param_grads accumulate",
          prep=lambda: put1(og, start))
    check(og.get()[0], start + P[0].sum(0), bnd(0) + U32 * np.abs(start + P[0].sum(0)), f"ln_param_grads/f32 dgamma accumulate: {name}")
    ob.check_canary(name + ": a NULL dbeta", torch.zeros(1, W, dtype=torch.bool))
    og.check_canary(name)


def test_ln_param_grads_grouped(dev):
    """ten items (two launches) of different widths and block counts (130 blocks: the second trip of the 128-block loop), overwrite
    and accumulate, a NULL dgamma or a NULL dbeta leaving the other item's outputs untouched"""
    from mic_amd import ops

    rng = np.random.default_rng(3)
    shapes = [(1, 8), (3, 40), (130, 768), (7, 1032), (512, 64), (9, 2048), (2, 24), (128, 32), (129, 16), (5, 520)]
    items, chk = [], []
    for i, (nblk, W) in enumerate(shapes):
        P = rng.standard_normal((2 * nblk, W)).astype(np.float32).astype(np.float64)
        pb = Buf(2 * nblk, W, W, F32, dev, "nan", off=4).put(P)
        og, ob = vec(W, dev), vec(W, dev)
        acc, nog, nob = i % 3 == 1, i == 4, i == 6
        start = rng.standard_normal((2, W)).astype(np.float32).astype(np.float64)
        items.append((pb.t, nblk, W, None if nog else og.t[0], None if nob else ob.t[0], acc))
        chk.append((P.reshape(2, nblk, W), og, ob, acc, nog, nob, start, nblk, W, pb))
    outs = [o for t in chk for o in (t[1], t[2])]

    def prep():
        for _, og, ob, acc, nog, nob, start, _, _, _ in chk:
            if acc and not nog:
                put1(og, start[0])
            if acc and not nob:
                put1(ob, start[1])

    twice(lambda: ops.ln_param_grads(items), outs, "ln_param_grads grouped", prep=prep)
    for i, (P, og, ob, acc, nog, nob, start, nblk, W, _) in enumerate(chk):
        for k, (o, null) in enumerate(((og, nog), (ob, nob))):
            if null:
                o.check_canary(f"item {i}: a NULL output's neighbour", torch.zeros(1, W, dtype=torch.bool))
                continue
            o.check_canary(f"item {i}")
            ref = P[k].sum(0) + (start[k] if acc else 0.0)
            check(o.get()[0], ref, gamma_k(nblk) * np.abs(P[k]).sum(0) + U32 * np.abs(ref) + 1e-300,
                  f"ln_param_grads/f32 {'dbeta' if k else 'dgamma'}: item {i} {nblk}x{W}")


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("N,K,bias", RC.LN_FOLD)
def test_ln_fold_weight(dev, N, K, bias, dtype):
    from mic_amd import ops

    dt = TD[dtype]
    rng = np.random.default_rng(N + K)
    w = round_to(rng.standard_normal((N, K)), dtype)
    g, be, bi = ((s * rng.standard_normal(n)).astype(np.float32).astype(np.float64) + o for s, n, o in ((0.2, K, 1.0), (0.2, K, 0.0), (1.0, N, 0.0)))
    wd = Buf(N, K, K + 8, dt, dev, "nan").put(w)
    gd, bed, bid = put1(vec(K, dev, "nan"), g), put1(vec(K, dev, "nan"), be), put1(vec(N, dev, "nan"), bi)
    wf, cs, bf = Buf(N, K, K + 16, dt, dev, "canary"), vec(N, dev), vec(N, dev)
    twice(lambda: ops.ln_fold_weight(wd.t, gd.t[0], bed.t[0], bid.t[0] if bias else None, wf.t, cs.t[0], bf.t[0]), [wf, cs, bf], "ln_fold_weight")
    for o in (wf, cs, bf):
        o.check_canary("ln_fold_weight")
    r_wf, r_cs, e_cs, r_bf, e_bf = RR.fold_ref(w, g, be, bi if bias else None, dtype)
    assert np.array_equal(wf.get(), r_wf), "w_fold is not round(w * gamma) bit for bit"
    what = f"{N}x{K}{' bias' if bias else ''}"
    check(cs.get()[0], r_cs, e_cs, f"ln_fold_weight/{dtype} colsum: {what}")
    check(bf.get()[0], r_bf, e_bf, f"ln_fold_weight/{dtype} bias_fold: {what}")


# ------------------------------------------------------------------------------------------------ cross-entropy
@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("ls", RC.CE_LS)
@pytest.mark.parametrize("name", [c["name"] for c in RC.CE])
def test_ce(dev, name, ls, dtype):
    """mic_ce_rows -> mic_ce_reduce -> mic_ce_bwd (loss_scale 4) on the device's own row_lse / denom"""
    from mic_amd import ops

    c, dt = RC.CE_BY[name], TD[dtype]
    rows, V, Vpad, ld = c["rows"], c["V"], c["Vpad"], c["ld"]
    x, labels, mask = RC.ce_inputs(c, dtype)
    lg = Buf(rows, V, ld, dt, dev, "nan").put(x)
    ld_, md = ints(labels, dev), ints(mask, dev)
    lse, rl = vec(rows, dev), vec(rows, dev)
    twice(lambda: ops.ce_rows(lg.t, ld, V, ld_, md, ls, lse.t[0], rl.t[0], rows), [lse, rl], name)
    lse.check_canary(name)
    rl.check_canary(name)
    r = RR.ce_rows_ref(x, labels, ls)
    glse, gl = lse.get()[0], rl.get()[0]
    check(glse, r["lse"], r["bound_lse"], f"ce_rows/{dtype} row_lse: {name}")
    if c.get("neginf") and ls > 0:  # the smoothed loss of a row with a -inf logit is +inf
        inf = np.isinf(x).any(1)
        assert np.array_equal(np.isposinf(gl), inf)
        check(gl[~inf], r["loss"][~inf], r["bound_loss"][~inf], f"ce_rows/{dtype} row_loss ls={ls}: {name}")
        put1(rl, np.where(inf, 0.0, gl))
    else:
        check(gl, r["loss"], r["bound_loss"], f"ce_rows/{dtype} row_loss ls={ls}: {name}")
    loss, den = vec(1, dev), vec(1, dev)
    twice(lambda: ops.ce_reduce(rl.t[0], md, loss.t[0], den.t[0], rows), [loss, den], name + " reduce")
    loss.check_canary(name)
    den.check_canary(name)
    rloss, eloss, rden = RR.ce_reduce_ref(rl.get()[0], mask)
    assert den.get()[0, 0] == rden == mask.sum(), "denom is not the exact count"
    check(loss.get()[0], [rloss], [eloss], f"ce_reduce/f32 loss: {name}")
    # backward in place: x in [0, V), NaN in [V, Vpad), canary in [Vpad, ld) and in the rows behind
    gb = Buf(rows, Vpad, ld, dt, dev, "canary")
    pad = np.full((rows, Vpad - V), np.nan)
    twice(lambda: ops.ce_bwd(gb.t, ld, V, Vpad, ld_, md, ls, lse.t[0], den.t[0], rows, loss_scale=4.0), [gb], name + " bwd",
          prep=lambda: gb.put(x).put(pad, V) if Vpad > V else gb.put(x))
    gb.check_canary(name + " dlogits")
    xp = np.zeros((rows, Vpad))
    xp[:, :V] = x
    v, e = RR.ce_bwd_ref(xp, V, labels, mask, ls, glse, rden, 4.0, dtype)
    got = gb.get()
    check(got, v, e, f"ce_bwd/{dtype} dlogits ls={ls}: {name}")
    assert zero_bits(gb.t[:, V:]) if Vpad > V else True, f"{name}: padding columns V .. Vpad are not exact zeros"
    assert zero_bits(gb.t[md == 0]), f"{name}: the gradient of a masked row is not all zero bits"
    if c.get("neginf"):
        w = 4.0 / rden
        low = float(np.float32(ls)) / (V - 1) if ls > 0 else 0.0
        at = np.isneginf(x) & (mask != 0)[:, None]
        assert at.any() and np.allclose(got[:, :V][at], -w * low, rtol=2.0 ** -7, atol=0), f"{name}: an entry at -inf is not w (0 - low)"


@pytest.mark.parametrize("rows", [24, 300, 1000])
def test_ce_reduce_zero_weight_rows(dev, rows):
    """rows of weight 0 carry a row_loss of 3e38: they contribute exactly nothing; 300 and 1000 rows take the stride loop"""
    from mic_amd import ops

    rng = np.random.default_rng(rows)
    mask = (rng.random(rows) < 0.6).astype(np.int32)
    mask[0], mask[-1] = 1, 0
    rl = np.where(mask != 0, rng.random(rows) * 10, 3e38).astype(np.float32).astype(np.float64)
    rld, md = put1(vec(rows, dev, "nan"), rl), ints(mask, dev)
    loss, den = vec(1, dev), vec(1, dev)
    twice(lambda: ops.ce_reduce(rld.t[0], md, loss.t[0], den.t[0], rows), [loss, den], "ce_reduce")
    ref, e, rden = RR.ce_reduce_ref(np.where(mask != 0, rl, 0.0), mask)
    assert den.get()[0, 0] == rden
    check(loss.get()[0], [ref], [e], f"ce_reduce/f32 loss: zero weights, {rows} rows")


@pytest.mark.parametrize("dtype", RC.DTYPES)
@pytest.mark.parametrize("layout", RC.TILES_LAYOUT)
@pytest.mark.parametrize("V", RC.CE_TILES)
def test_ce_rows_tiles(dev, V, layout, dtype):
    """the (max, sum exp) partials built here in fp64 from the stored logits and rounded to fp32 (no GEMM); row 1 has a granule of
    (-inf, 0); entries ntiles .. stat_ld of every row hold NaN"""
    from mic_amd import ops

    dt, rows = TD[dtype], 6
    rng = np.random.default_rng(V)
    x = round_to(rng.standard_normal((rows, V)) * 3, dtype)
    x[1, 64:128] = -np.inf
    labels = RC.ce_labels(rows, V)
    labels[1] = 3
    part = RR.tile_partials(x)
    nt = part.shape[1]
    ld = (V + 7) // 8 * 8 + 8
    lg = Buf(rows, V, ld, dt, dev, "nan").put(x)
    stat_ld = nt + 2 + (nt % 2) if layout != "odd_ld" else nt + 1 + (nt % 2)
    assert stat_ld % 2 == (layout == "odd_ld")
    flat = torch.full(((rows + 1) * 2 * stat_ld + 8,), float("nan"), dtype=F32, device=dev)
    off = 2 if layout == "base8" else 0
    st = flat[off:off + rows * 2 * stat_ld].view(rows, 2 * stat_ld)
    assert st.data_ptr() % 16 == (8 if layout == "base8" else 0)
    st[:, :2 * nt] = torch.from_numpy(part.reshape(rows, 2 * nt)).to(dev)
    lse, rl = vec(rows, dev), vec(rows, dev)
    ld_ = ints(labels, dev)
    twice(lambda: ops.ce_rows_tiles(lg.t, ld, V, st, ld_, lse.t[0], rl.t[0], rows), [lse, rl], f"ce_rows_tiles {V} {layout}")
    lse.check_canary("row_lse")
    rl.check_canary("row_loss")
    r = RR.ce_tiles_ref(part, x[np.arange(rows), labels])
    check(lse.get()[0], r["lse"], r["bound_lse"], f"ce_rows_tiles/{dtype} row_lse: V={V} {layout}")
    check(rl.get()[0], r["loss"], r["bound_loss"], f"ce_rows_tiles/{dtype} row_loss: V={V} {layout}")


@pytest.mark.parametrize("ls", RC.CE_LS)
@pytest.mark.parametrize("name", [c["name"] for c in RC.CE_T])
def test_ce_bwd_t_and_transpose(dev, name, ls):
    """mic_ce_bwd_t (bf16): the in-place dlogits under the bound of mic_ce_bwd and with its bits; dlogits_t bit for bit the transpose
    of the dlogits just stored, columns rows .. rows_pad zeros, rows_pad .. ld_t canary; colsum = a non-zero start + the sum of the
    stored values; mic_transpose_bf16 of the stored dlogits gives the same bits"""
    from mic_amd import ops

    c = next(t for t in RC.CE_T if t["name"] == name)
    rows, V, Vpad, ld, ld_t, dt = c["rows"], c["V"], c["Vpad"], c["ld"], c["ld_t"], torch.bfloat16
    rp = c["rows_pad"] or (rows + 63) // 64 * 64
    x, labels, mask = RC.ce_inputs(dict(c, mask="alt"), "bf16")
    ld_, md = ints(labels, dev), ints(mask, dev)
    lse_ref = RR.ce_rows_ref(x, labels, ls)["lse"].astype(np.float32).astype(np.float64)
    lsed, dend = put1(vec(rows, dev, "nan"), lse_ref), put1(vec(1, dev, "nan"), [float(mask.sum())])
    gb, gt, cs = Buf(rows, Vpad, ld, dt, dev, "canary"), Buf(Vpad, rp, ld_t, dt, dev, "canary"), vec(Vpad, dev)
    start = np.linspace(-2, 2, Vpad).astype(np.float32).astype(np.float64) + 0.25
    pad = np.full((rows, Vpad - V), np.nan)

    def prep():
        gb.put(x)
        if Vpad > V:
            gb.put(pad, V)
        put1(cs, start)

    twice(lambda: ops.ce_bwd_t(gb.t, ld, V, Vpad, ld_, md, ls, lsed.t[0], dend.t[0], rows, gt.t, rows_pad=c["rows_pad"], colsum=cs.t[0],
                               loss_scale=4.0), [gb, gt, cs], name, prep=prep, inexact=[cs])
    for o in (gb, gt, cs):
        o.check_canary(name)
    xp = np.zeros((rows, Vpad))
    xp[:, :V] = x
    v, e = RR.ce_bwd_ref(xp, V, labels, mask, ls, lse_ref, float(mask.sum()), 4.0, "bf16")
    got = gb.get()
    check(got, v, e, f"ce_bwd_t/bf16 dlogits ls={ls}: {name}")
    assert (Vpad == V or zero_bits(gb.t[:, V:])) and zero_bits(gb.t[md == 0])
    tb = gt.full[:Vpad].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    RR.check_transposed(tb, bits16(gb), rows, rp)
    ref_cs = start + got.sum(0)
    check(cs.get()[0], ref_cs, (gamma_k(rows) + U32) * (np.abs(got).sum(0) + np.abs(start)) + 1e-300, f"ce_bwd_t/bf16 colsum ls={ls}: {name}")
    g2 = Buf(rows, Vpad, ld, dt, dev, "canary").put(x)
    if Vpad > V:
        g2.put(pad, V)
    ops.ce_bwd(g2.t, ld, V, Vpad, ld_, md, ls, lsed.t[0], dend.t[0], rows, loss_scale=4.0)
    assert torch.equal(g2.bits(), gb.bits()), f"{name}: mic_ce_bwd_t and mic_ce_bwd store different dlogits"
    t2 = Buf(Vpad, rp, ld_t, dt, dev, "canary")
    twice(lambda: ops.transpose_bf16(gb.t, t2.t, rows, Vpad, rows_pad=c["rows_pad"]), [t2], name + " transpose")
    assert torch.equal(t2.bits(), gt.bits()), f"{name}: mic_transpose_bf16 of the stored dlogits differs from dlogits_t"


# ------------------------------------------------------------------------------------------------ AdamW
def _adamw_bufs(n, dev, p, m, v, g, lp=True):
    pb, mb, vb = vec(n, dev), vec(n, dev), vec(n, dev)
    gb = put1(vec(n, dev, "nan"), g)
    lpb = vec(n, dev, dtype=torch.bfloat16) if lp else None
    src = [torch.from_numpy(a.reshape(1, -1)).to(F32).to(dev) for a in (p, m, v)]

    def prep():
        for b, s in zip((pb, mb, vb), src):
            b.t.copy_(s)

    return pb, mb, vb, gb, lpb, prep


@pytest.mark.parametrize("name", [c["name"] for c in RC.ADAMW])
def test_adamw(dev, name):
    from mic_amd import ops

    c = RC.ADAMW_BY[name]
    n, h = c["n"], RC.adamw_hyper(c)
    p, m, v, g = RC.adamw_inputs(c)
    pb, mb, vb, gb, lpb, prep = _adamw_bufs(n, dev, p, m, v, g, lp=not c.get("nolp"))
    hy = torch.tensor([h["lr"], h["t"]], dtype=F32, device=dev)
    outs = [o for o in (pb, mb, vb, lpb) if o is not None]
    twice(lambda: ops.adamw(pb.t[0], mb.t[0], vb.t[0], gb.t[0], lpb.t[0] if lpb else None, hy, h["b1"], h["b2"], h["eps"], h["wd"],
                            grad_scale=h["gscale"], n=n), outs, name, prep=prep)
    for o in outs:
        o.check_canary(name)
    idx = np.arange(n) if n <= 10000 else np.unique(np.concatenate([np.arange(4100), np.arange(n - 4100, n),
                                                                    np.random.default_rng(1).integers(n, size=100000)]))
    r = RR.adamw_ref(p[idx], m[idx], v[idx], g[idx], **h)
    for b, k in ((pb, "p"), (mb, "m"), (vb, "v")):
        got = b.t[0].double().cpu().numpy()
        assert np.isfinite(got).all(), f"{name}: {k} not finite"
        check(got[idx], r[k], r["bound_" + k], f"adamw/f32 {k}: {name}")
    if lpb:
        assert torch.equal(lpb.t[0], pb.t[0].to(torch.bfloat16)), f"{name}: p_lp is not the bf16 rounding of the stored p"
    if c["lr"] == 0:
        assert np.array_equal(pb.t[0].cpu().numpy(), p.astype(np.float32)), f"{name}: lr = 0 moved p"
        assert not np.array_equal(mb.t[0].cpu().numpy(), m.astype(np.float32))


@pytest.mark.parametrize("want", [0, 1])
@pytest.mark.parametrize("flags", RC.ADAMW_FLAGS)
@pytest.mark.parametrize("rows,width", RC.ADAMW_ROWS)
def test_adamw_rows(dev, rows, width, flags, want):
    """the selected rows within the bounds, p_lp the rounding of the stored p; the other rows keep their bits in p, m, v and p_lp"""
    from mic_amd import ops

    c = RC.ADAMW_BY["adamw_4100_t7"]
    n, h = rows * width, RC.adamw_hyper(c)
    p, m, v, g = RC.adamw_inputs(c, n)
    fl = {"none": np.zeros(rows), "all": np.ones(rows), "mixed": np.arange(rows) % 2}[flags].astype(np.uint8)
    fl = fl * (1 + np.arange(rows) % 3).astype(np.uint8)  # any non-zero byte is a set flag
    sel = np.repeat((fl != 0) == (want != 0), width)
    pb, mb, vb, gb, lpb, prep = _adamw_bufs(n, dev, p, m, v, g)
    hy = torch.tensor([h["lr"], h["t"]], dtype=F32, device=dev)
    fd = ints(fl, dev, torch.uint8)
    outs = [pb, mb, vb, lpb]
    twice(lambda: ops.adamw_rows(rows, width, fd, want, pb.t[0], mb.t[0], vb.t[0], gb.t[0], lpb.t[0], hy, h["b1"], h["b2"], h["eps"], h["wd"],
                                 grad_scale=h["gscale"]), outs, f"adamw_rows {rows}x{width}", prep=prep)
    for o in (pb, mb, vb):
        o.check_canary("adamw_rows")
    lpb.check_canary("adamw_rows p_lp: rows that were not selected", torch.from_numpy(sel.reshape(1, -1)))
    r = RR.adamw_ref(p, m, v, g, **h)
    sd = torch.from_numpy(sel).to(dev)
    for b, k, a in ((pb, "p", p), (mb, "m", m), (vb, "v", v)):
        got = b.t[0].double().cpu().numpy()
        assert np.array_equal(got[~sel], a[~sel]), f"{k} of a row that was not selected moved"
        if sel.any():
            check(got[sel], r[k][sel], r["bound_" + k][sel], f"adamw_rows/f32 {k}: {rows}x{width} {flags} want={want}")
    assert torch.equal(lpb.t[0][sd], pb.t[0].to(torch.bfloat16)[sd])


# ------------------------------------------------------------------------------------------------ refusals
def test_rowop_refusals(dev):
    """every MIC_CHECK condition of the entry points in scope: MicError on the host, the canary-filled outputs untouched"""
    from mic_amd import ops

    bf = torch.bfloat16
    mk = lambda fill, rows, cols, ld, dt=bf: Buf(rows, cols, ld, dt, dev, fill)  # noqa: E731
    R = 4
    for W in (12, 2056):  # width % 8, width > 2048
        x, dy = mk("nan", R, W, W).put(np.ones((R, W))), mk("nan", R, W, W).put(np.ones((R, W)))
        g = put1(vec(W, dev, "nan"), np.ones(W))
        y, dx, mean, rstd, dg, part = mk("canary", R, W, W), mk("canary", R, W, W), vec(R, dev), vec(R, dev), vec(W, dev), mk("canary", 2, W, W, F32)
        _refused(lambda: ops.layernorm_fwd(x.t, g.t[0], g.t[0], 1e-5, y.t, mean.t[0], rstd.t[0], rows=R), [y, mean, rstd], f"ln_fwd width {W}")
        put1(mean, np.zeros(R))
        put1(rstd, np.ones(R))
        _refused(lambda: ops.layernorm_bwd(x.t, g.t[0], mean.t[0], rstd.t[0], dy.t, dx.t, dg.t[0], None, rows=R), [dx, dg], f"ln_bwd width {W}")
        _refused(lambda: ops.layernorm_bwd_partials(x.t, g.t[0], mean.t[0], rstd.t[0], dy.t, dx.t, part.t, rows=R), [dx, part], f"ln_bwd_partials width {W}")
    W = 64
    x, dy, g = mk("nan", R, W, W).put(np.ones((R, W))), mk("nan", R, W, W).put(np.ones((R, W))), put1(vec(W, dev, "nan"), np.ones(W))
    st, dx = put1(vec(R, dev, "nan"), np.ones(R)), mk("canary", R, W, W)
    _refused(lambda: ops.layernorm_bwd_partials(x.t, g.t[0], st.t[0], st.t[0], dy.t, dx.t, None, rows=R), [dx], "ln_bwd_partials partials NULL")
    wf, cs = mk("canary", R, W, W + 8), vec(R, dev)
    _refused(lambda: ops.ln_fold_weight(x.t[:, :12], g.t[0], g.t[0], None, wf.t[:, :12], cs.t[0], cs.t[0]), [wf, cs], "ln_fold_weight K 12")
    # cross-entropy
    rows, V, Vpad, ld = 4, 40, 40, 48
    lg = mk("canary", rows, Vpad, ld)
    lab, msk = ints(np.zeros(rows), dev), ints(np.ones(rows), dev)
    lse, rl, den = vec(rows, dev), vec(rows, dev), put1(vec(1, dev, "nan"), [4.0])
    stat = torch.zeros(rows, 4, device=dev)
    _refused(lambda: ops.ce_rows(lg.t, ld, 1, lab, msk, 0.0, lse.t[0], rl.t[0], rows), [lse, rl], "ce_rows V 1")
    _refused(lambda: ops.ce_rows(lg.t, 32, V, lab, msk, 0.0, lse.t[0], rl.t[0], rows), [lse, rl], "ce_rows ld < V")
    _refused(lambda: ops.ce_rows_tiles(lg.t, ld, 1, stat, lab, lse.t[0], rl.t[0], rows), [lse, rl], "ce_rows_tiles V 1")
    _refused(lambda: ops.ce_rows_tiles(lg.t, 32, V, stat, lab, lse.t[0], rl.t[0], rows), [lse, rl], "ce_rows_tiles ld < V")
    _refused(lambda: ops.ce_rows_tiles(lg.t, ld, 200, stat, lab, lse.t[0], rl.t[0], rows), [lse, rl], "ce_rows_tiles stat_ld < ntiles")
    lsev = put1(vec(rows, dev, "nan"), np.ones(rows))
    gt = mk("canary", Vpad, 64, 72)
    _refused(lambda: ops.ce_bwd(lg.t, ld, 1, Vpad, lab, msk, 0.0, lsev.t[0], den.t[0], rows), [lg], "ce_bwd V 1")
    _refused(lambda: ops.ce_bwd(lg.t, ld, V - 3, V - 3, lab, msk, 0.0, lsev.t[0], den.t[0], rows), [lg], "ce_bwd Vpad % 8")
    _refused(lambda: ops.ce_bwd(lg.t, 32, V, Vpad, lab, msk, 0.0, lsev.t[0], den.t[0], rows), [lg], "ce_bwd ld < Vpad")
    bt = lambda **kw: ops.ce_bwd_t(*[kw.get("lg", lg.t), kw.get("ld", ld), kw.get("V", V), kw.get("Vpad", Vpad), lab, msk, 0.0, lsev.t[0],  # noqa: E731
                                     den.t[0], rows, kw.get("gt", gt.t)], rows_pad=kw.get("rows_pad", 0))
    _refused(lambda: bt(V=1), [lg, gt], "ce_bwd_t V 1")
    _refused(lambda: bt(V=37, Vpad=37), [lg, gt], "ce_bwd_t Vpad % 8")
    _refused(lambda: bt(ld=32), [lg, gt], "ce_bwd_t ld < Vpad")
    _refused(lambda: bt(rows_pad=100), [lg, gt], "ce_bwd_t rows_pad % 64")
    _refused(lambda: bt(rows_pad=128), [lg, gt], "ce_bwd_t ld_t < rows_pad")
    _refused(lambda: bt(lg=lg.full[:rows, 4:4 + Vpad]), [lg, gt], "ce_bwd_t logits 8 B into a 16-B line")
    _refused(lambda: bt(gt=gt.full[:Vpad, 4:68]), [lg, gt], "ce_bwd_t dlogits_t 8 B into a 16-B line")
    _refused(lambda: ops.transpose_bf16(lg.t, gt.t, rows, Vpad, rows_pad=100), [gt], "transpose rows_pad % 64")
    _refused(lambda: ops.transpose_bf16(lg.t, gt.full[:Vpad, 4:68], rows, Vpad), [gt], "transpose misaligned dst")
    # AdamW
    n = 8
    p, m, v = vec(n, dev), vec(n, dev), vec(n, dev)
    gr, hy = put1(vec(n, dev, "nan"), np.ones(n)), torch.tensor([1e-3, 1.0], device=dev)
    _refused(lambda: ops.adamw(p.t[0], m.t[0], v.t[0], gr.t[0], None, hy, 0.9, 0.999, 1e-6, 0.01, n=6), [p, m, v], "adamw n % 4")
    fl = ints(np.ones(1), dev, torch.uint8)
    _refused(lambda: ops.adamw_rows(1, 6, fl, 1, p.t[0], m.t[0], v.t[0], gr.t[0], None, hy, 0.9, 0.999, 1e-6, 0.01), [p, m, v], "adamw_rows width % 4")
    _refused(lambda: ops.adamw_rows(1, 8, None, 1, p.t[0], m.t[0], v.t[0], gr.t[0], None, hy, 0.9, 0.999, 1e-6, 0.01), [p, m, v], "adamw_rows flags NULL")
