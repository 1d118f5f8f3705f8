"""The weighted cross-entropy entry points (mic_ce_reduce_w, mic_ce_bwd_w, mic_ce_bwd_t_w; csrc/elementwise.hip) on the MI355X
against the fp64 references and bounds of tests/util_loss_weights_ref.py, in the manner of tests/test_rowop_conformance_gpu.py:
outputs are windows in canary-filled allocations, padding columns hold NaN going in.  The weights of every case are distinct per row
and include +0, -0, negatives, a value above 1 and a nonzero weight on a row of mask 0.  row_weight = NULL and weights of 1.0 must
give the bits of the unweighted entry points."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_loss_weights_ref as LW  # noqa: E402
import util_rowop_cases as RC  # noqa: E402
import util_rowop_ref as RR  # noqa: E402
from test_attn_conformance_gpu import TD, Buf, _refused  # noqa: E402
from test_rowop_conformance_gpu import bits16, ints, put1, twice, vec, zero_bits  # noqa: E402
from util_gemm_ref import U32, check, gamma_k  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = torch.float32


def f32(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)


def test_ce_reduce_w(dev):
    """300 rows: the 256-thread stride loop takes a second trip"""
    from mic_amd import ops

    rows = 300
    rng = np.random.default_rng(rows)
    mask = (rng.random(rows) < 0.7).astype(np.int32)
    mask[0], mask[-1], mask[257] = 1, 0, 1
    w, _ = LW.kernel_weights(rows, mask, seed=1)
    rl = (rng.random(rows) * 10).astype(np.float32).astype(np.float64)
    rld, md, wd = put1(vec(rows, dev, "nan"), rl), ints(mask, dev), f32(w, dev)
    loss, den = vec(1, dev), vec(1, dev)
    twice(lambda: ops.ce_reduce(rld.t[0], md, loss.t[0], den.t[0], rows, row_weight=wd), [loss, den], "ce_reduce_w")
    loss.check_canary("ce_reduce_w loss")
    den.check_canary("ce_reduce_w denom")
    ref, e, rden = LW.ce_reduce_w_ref(rl, mask, w)
    print(f"[ce_reduce_w] loss {loss.get()[0, 0]:.7f} ref {ref:.7f} bound {e:.2e} denom {den.get()[0, 0]}")
    assert den.get()[0, 0] == rden == mask.sum(), "denom is not the exact mask count"
    check(loss.get()[0], [ref], [e], "ce_reduce_w/f32 loss")
    assert abs(ref - RR.ce_reduce_ref(rl, mask)[0]) > 1e-2  # (the weights are felt)
    wbits = (loss.bits(), den.bits())
    # NULL and weights of 1.0: the bits of mic_ce_reduce
    outs = {}
    for form, kw in (("plain", {}), ("null", dict(row_weight=None)), ("ones", dict(row_weight=torch.ones(rows, device=dev)))):
        for o in (loss, den):
            o.refill()
        ops.ce_reduce(rld.t[0], md, loss.t[0], den.t[0], rows, **kw)
        torch.cuda.synchronize()
        outs[form] = (loss.bits(), den.bits())
    for form in ("null", "ones"):
        assert all(torch.equal(a, b) for a, b in zip(outs[form], outs["plain"])), f"ce_reduce_w {form}: not the bits of mic_ce_reduce"
    assert not torch.equal(wbits[0], outs["plain"][0])


def _bwd_case(rows, V, dtype, mask, seed):
    x, labels, _ = RC.ce_inputs(dict(rows=rows, V=V, mask="ones"), dtype)
    w, zero_rows = LW.kernel_weights(rows, mask, seed=seed)
    return x, labels, np.asarray(mask, np.int32), w, zero_rows


@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_ce_bwd_w(dev, dtype, ls):
    """1026 chunks: one trip of 256 x 4 chunks plus a tail trip, padding columns V .. Vpad, ld > Vpad"""
    from mic_amd import ops

    rows, V, Vpad, ld, dt = 5, 8203, 8208, 8216, TD[dtype]
    x, labels, mask, w, zero_rows = _bwd_case(rows, V, dtype, [1, 1, 0, 1, 1], seed=2)
    ld_, md, wd = ints(labels, dev), ints(mask, dev), f32(w, dev)
    lse = RR.ce_rows_ref(x, labels, ls)["lse"].astype(np.float32).astype(np.float64)
    lsed, dend = put1(vec(rows, dev, "nan"), lse), put1(vec(1, dev, "nan"), [float(mask.sum())])
    gb = Buf(rows, Vpad, ld, dt, dev, "canary")
    pad = np.full((rows, Vpad - V), np.nan)
    prep = lambda: gb.put(x).put(pad, V)  # noqa: E731
    name = f"ce_bwd_w/{dtype} ls={ls}"
    twice(lambda: ops.ce_bwd(gb.t, ld, V, Vpad, ld_, md, ls, lsed.t[0], dend.t[0], rows, loss_scale=4.0, row_weight=wd), [gb], name, prep=prep)
    gb.check_canary(name)
    xp = np.zeros((rows, Vpad))
    xp[:, :V] = x
    v, e = LW.ce_bwd_w_ref(xp, V, labels, mask, w, ls, lse, float(mask.sum()), 4.0, dtype)
    got = gb.get()
    print(f"[{name}] worst |got - ref| / bound {np.max(np.abs(got - v) / np.maximum(e, 1e-300)):.3f}")
    check(got, v, e, f"{name} dlogits")
    assert zero_bits(gb.t[:, V:]), f"{name}: padding columns V .. Vpad are not +0"
    zr = torch.from_numpy(zero_rows).to(dev)
    assert int(zr.sum()) == 3 and zero_bits(gb.t[zr]), f"{name}: a row of mask 0, weight +0 or weight -0 is not +0 bits everywhere"
    assert not zero_bits(gb.t[~zr][:, :V])
    wbits = gb.bits()
    # NULL and weights of 1.0: the bits of mic_ce_bwd
    outs = {}
    for form, kw in (("plain", {}), ("null", dict(row_weight=None)), ("ones", dict(row_weight=torch.ones(rows, device=dev)))):
        gb.refill()
        prep()
        ops.ce_bwd(gb.t, ld, V, Vpad, ld_, md, ls, lsed.t[0], dend.t[0], rows, loss_scale=4.0, **kw)
        torch.cuda.synchronize()
        outs[form] = gb.bits()
    assert torch.equal(outs["null"], outs["plain"]) and torch.equal(outs["ones"], outs["plain"]), f"{name}: not the bits of mic_ce_bwd"
    assert not torch.equal(wbits, outs["plain"])


@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_ce_bwd_t_w(dev, ls):
    """70 rows in 128: the second 64-row tile is partly filled; 1008 columns: the second 512-column tile is partial"""
    from mic_amd import ops

    rows, rp, V, Vpad, ld, ld_t, dt = 70, 128, 1003, 1008, 1016, 136, torch.bfloat16
    mask = (np.arange(rows) % 3 != 2).astype(np.int32)
    x, labels, mask, w, zero_rows = _bwd_case(rows, V, "bf16", mask, seed=3)
    assert (zero_rows[:64].any() and zero_rows[64:].any()) and (w[64:] != 0).any()
    ld_, md, wd = ints(labels, dev), ints(mask, dev), f32(w, dev)
    lse = RR.ce_rows_ref(x, labels, ls)["lse"].astype(np.float32).astype(np.float64)
    lsed, dend = put1(vec(rows, dev, "nan"), lse), put1(vec(1, dev, "nan"), [float(mask.sum())])
    gb, gt, cs = Buf(rows, Vpad, ld, dt, dev, "canary"), Buf(Vpad, rp, ld_t, dt, dev, "canary"), vec(Vpad, dev)
    start = np.linspace(-2, 2, Vpad).astype(np.float32).astype(np.float64) + 0.25
    pad = np.full((rows, Vpad - V), np.nan)

    def prep():
        gb.put(x).put(pad, V)
        put1(cs, start)

    name = f"ce_bwd_t_w ls={ls}"
    run = lambda **kw: ops.ce_bwd_t(gb.t, ld, V, Vpad, ld_, md, ls, lsed.t[0], dend.t[0], rows, gt.t, rows_pad=rp, colsum=cs.t[0],  # noqa: E731
                                    loss_scale=4.0, **kw)
    twice(lambda: run(row_weight=wd), [gb, gt, cs], name, prep=prep, inexact=[cs])
    for o in (gb, gt, cs):
        o.check_canary(name)
    # the in-place dlogits: the bits of mic_ce_bwd_w
    g2 = Buf(rows, Vpad, ld, dt, dev, "canary").put(x).put(pad, V)
    ops.ce_bwd(g2.t, ld, V, Vpad, ld_, md, ls, lsed.t[0], dend.t[0], rows, loss_scale=4.0, row_weight=wd)
    torch.cuda.synchronize()
    assert torch.equal(g2.bits(), gb.bits()), f"{name}: mic_ce_bwd_t_w and mic_ce_bwd_w store different dlogits"
    xp = np.zeros((rows, Vpad))
    xp[:, :V] = x
    v, e = LW.ce_bwd_w_ref(xp, V, labels, mask, w, ls, lse, float(mask.sum()), 4.0, "bf16")
    got = gb.get()
    check(got, v, e, f"{name} dlogits")
    zr = torch.from_numpy(zero_rows).to(dev)
    assert zero_bits(gb.t[:, V:]) and zero_bits(gb.t[zr]) and not zero_bits(gb.t[~zr][:, :V])
    # the transposed copy: bit for bit, zero padding columns
    tb = gt.full[:Vpad].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    RR.check_transposed(tb, bits16(gb), rows, rp)
    # colsum: start + the sum of the STORED (weighted) values
    check(cs.get()[0], start + got.sum(0), (gamma_k(rows) + U32) * (np.abs(got).sum(0) + np.abs(start)) + 1e-300, f"{name} colsum")
    wbits = (gb.bits(), gt.bits())
    # weights of 1.0 (and NULL): the bits of mic_ce_bwd_t
    outs = {}
    for form, kw in (("plain", {}), ("null", dict(row_weight=None)), ("ones", dict(row_weight=torch.ones(rows, device=dev)))):
        for o in (gb, gt, cs):
            o.refill()
        prep()
        run(**kw)
        torch.cuda.synchronize()
        outs[form] = (gb.bits(), gt.bits())
        plain_cs = cs.get()[0] if form == "plain" else plain_cs
        check(cs.get()[0], plain_cs, 2 * (gamma_k(rows) + U32) * (np.abs(gb.get()).sum(0) + np.abs(start)) + 1e-300, f"{name} colsum {form}")
    for form in ("null", "ones"):
        assert all(torch.equal(a, b) for a, b in zip(outs[form], outs["plain"])), f"{name} {form}: not the bits of mic_ce_bwd_t"
    assert not torch.equal(wbits[0], outs["plain"][0])


def test_weighted_refusals(dev):
    """the MIC_CHECK conditions of the unweighted entry points (test_rowop_refusals), with weights: MicError on the host, the
    canary-filled operands untouched"""
    from mic_amd import ops

    bf = torch.bfloat16
    rows, V, Vpad, ld = 4, 40, 40, 48
    lg = Buf(rows, Vpad, ld, bf, dev, "canary")
    lab, msk, wd = ints(np.zeros(rows), dev), ints(np.ones(rows), dev), f32(np.array([1.5, -1.0, 0.0, 2.0]), dev)
    den = put1(vec(1, dev, "nan"), [4.0])
    lsev = put1(vec(rows, dev, "nan"), np.ones(rows))
    gt = Buf(Vpad, 64, 72, bf, dev, "canary")
    loss, dout = vec(1, dev), vec(1, dev)
    _refused(lambda: ops.ce_reduce(lsev.t[0], msk, loss.t[0], dout.t[0], 0, row_weight=wd), [loss, dout], "ce_reduce_w rows 0")
    _refused(lambda: ops.ce_reduce(lsev.t[0], None, loss.t[0], dout.t[0], rows, row_weight=wd), [loss, dout], "ce_reduce_w mask NULL")
    _refused(lambda: ops.ce_bwd(lg.t, ld, 1, Vpad, lab, msk, 0.0, lsev.t[0], den.t[0], rows, row_weight=wd), [lg], "ce_bwd_w V 1")
    _refused(lambda: ops.ce_bwd(lg.t, ld, V - 3, V - 3, lab, msk, 0.0, lsev.t[0], den.t[0], rows, row_weight=wd), [lg], "ce_bwd_w Vpad % 8")
    _refused(lambda: ops.ce_bwd(lg.t, 32, V, Vpad, lab, msk, 0.0, lsev.t[0], den.t[0], rows, row_weight=wd), [lg], "ce_bwd_w ld < Vpad")
    bt = lambda **kw: ops.ce_bwd_t(*[kw.get("lg", lg.t), kw.get("ld", ld), kw.get("V", V), kw.get("Vpad", Vpad), lab, msk, 0.0, lsev.t[0],  # noqa: E731
                                     den.t[0], rows, kw.get("gt", gt.t)], rows_pad=kw.get("rows_pad", 0), row_weight=wd)
    _refused(lambda: bt(V=1), [lg, gt], "ce_bwd_t_w V 1")
    _refused(lambda: bt(V=37, Vpad=37), [lg, gt], "ce_bwd_t_w Vpad % 8")
    _refused(lambda: bt(ld=32), [lg, gt], "ce_bwd_t_w ld < Vpad")
    _refused(lambda: bt(rows_pad=100), [lg, gt], "ce_bwd_t_w rows_pad % 64")
    _refused(lambda: bt(rows_pad=128), [lg, gt], "ce_bwd_t_w ld_t < rows_pad")
    _refused(lambda: bt(lg=lg.full[:rows, 4:4 + Vpad]), [lg, gt], "ce_bwd_t_w logits 8 B into a 16-B line")
    _refused(lambda: bt(gt=gt.full[:Vpad, 4:68]), [lg, gt], "ce_bwd_t_w dlogits_t 8 B into a 16-B line")
    # weights of another type or too few of them never reach the library
    for bad in (wd.double(), wd[:3], torch.ones(8, device=dev)[::2]):
        lg.refill()
        with pytest.raises(ValueError, match="row_weight"):
            ops.ce_bwd(lg.t, ld, V, Vpad, lab, msk, 0.0, lsev.t[0], den.t[0], rows, row_weight=bad)
        torch.cuda.synchronize()
        lg.check_canary("row_weight refused", torch.zeros(rows, Vpad, dtype=torch.bool))
