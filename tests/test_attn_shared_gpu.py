"""One-tile cross-attention with keys / values shared by G query sequences (mic_attn_fwd_shared / mic_attn_bwd_shared) on the MI355X.

n_img = 2 images, H = 2 heads, G captions per image, dense rows and packed rows with ragged q_len (1 and Tq_max among them), both
storage types.  Per case:
  - out, lse and dq are bitwise those of the existing one-tile entry points (mic_attn_fwd / mic_attn_bwd, or the packed forms with
    kv_packed = 0) run on K / V rows replicated G times;
  - dk / dv against the fp64 reference per caption (tests/util_attn_ref.py: bwd_ref on the out / lse the backward was handed), summed
    over an image's captions in fp64.  The bound is the one tests/test_attn_conformance_gpu.py applies to the one-tile kernels' dK / dV,
    per caption, summed over the captions: the error of a sum is at most the sum of the errors — the kernel rounds the sum once where the
    bound allows a rounding per caption, and adds the captions in the same fp32 accumulator its contraction over the queries runs in;
  - G = 1: all five outputs bitwise those of the existing kernels;
  - every launch runs twice from freshly filled outputs: identical bits;
  - outputs are windows in canary-filled allocations (rows behind, a row stride wider than the heads' columns, an offset base): nothing
    outside the window, no lse slot behind q_len, and nothing at all by a refused call may change."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_attn_ref as AR  # noqa: E402
import util_gemm_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "f32": torch.float32}
IB = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
D, N_IMG, H = 64, 2, 2
HD = H * D
SHAPES = [(1, 1), (31, 50), (33, 50), (64, 64), (12, 50)]
GROUPS = [1, 2, 3, 5]


class Buf:
    """a [rows][cols] window with row stride ld, `off` elements into a flat allocation with `extra` rows and 8 elements behind it;
    fill 'nan' (an operand: nothing outside the window may be read) or 'canary' (an output: nothing outside may be written)"""

    def __init__(self, rows, cols, ld, dtype, dev, fill, off=8, extra=3):
        self.rows, self.cols, self.ld, self.off, self.fill = rows, cols, ld, off, fill
        self.flat = torch.empty(off + (rows + extra) * ld + 8, dtype=dtype, device=dev)
        self.full = self.flat[off:off + (rows + extra) * ld].view(rows + extra, ld)
        self.t = self.full[:rows, :cols]
        self.refill()

    def refill(self):
        if self.fill == "nan":
            self.flat.fill_(float("nan"))
        else:
            GR.sentinel_fill(self.flat)
        return self

    def put(self, x, c0=0):
        self.full[:self.rows, c0:c0 + x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x)).to(self.flat.device).to(self.flat.dtype)
        return self

    def cols_of(self, c0, n):
        return self.full[:self.rows, c0:c0 + n]

    def get(self, c0=0, n=None):
        return self.full[:self.rows, c0:c0 + (self.cols - c0 if n is None else n)].double().cpu().numpy()

    def bits(self):
        return self.flat.view(IB[self.flat.dtype]).clone()

    def check_canary(self, what, written=None):
        w = torch.zeros(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        win = w[self.off:self.off + self.full.numel()].view(self.full.shape)[:self.rows, :self.cols]
        win[...] = True if written is None else written.to(w.device)
        AR.check_canary_mask(self.flat, w, what)


def _twice(run, outs, what):
    for o in outs:
        o.refill()
    run()
    torch.cuda.synchronize()
    first = [o.bits() for o in outs]
    for o in outs:
        o.refill()
    run()
    torch.cuda.synchronize()
    for o, f in zip(outs, first):
        assert torch.equal(o.bits(), f), f"{what}: two runs differ"
    return first


def _q_len(B, Tm, packed):
    """dense: every sequence full; packed: ragged, with 1 and Tq_max among the lengths"""
    if not packed:
        return [Tm] * B
    cyc = [Tm, 1, max(1, Tm // 2), max(1, Tm - 1), min(Tm, 33), min(Tm, 2)]
    return [cyc[b % len(cyc)] for b in range(B)]


def _hd(x):
    """[T][H*64] -> [H][T][64]"""
    return x.reshape(x.shape[0], H, D).transpose(1, 0, 2)


@pytest.mark.parametrize("rows", ["dense", "packed"])
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("Tm,Tk", SHAPES)
@pytest.mark.parametrize("G", GROUPS)
def test_shared_against_the_one_tile_kernels_and_fp64(dev, G, Tm, Tk, dtype, rows):
    from mic_amd import ops

    dt, packed, B = TD[dtype], rows == "packed", N_IMG * G
    ql = _q_len(B, Tm, packed)
    q_off = np.concatenate(([0], np.cumsum(ql)[:-1])).astype(np.int32)
    total = int(sum(ql))
    rng = np.random.default_rng(1000 * G + 10 * Tm + Tk + (1 if packed else 0))
    q, do = (GR.round_to(rng.standard_normal((total, HD)), dtype) for _ in range(2))
    k, v = (GR.round_to(rng.standard_normal((N_IMG * Tk, HD)), dtype) for _ in range(2))
    rep = np.repeat(np.arange(N_IMG), G)                                   # caption -> image
    krep, vrep = (np.concatenate([x[i * Tk:(i + 1) * Tk] for i in rep]) for x in (k, v))
    what = f"G={G} Tq_max={Tm} Tk={Tk} {dtype} {rows}"

    qd = Buf(total, HD, HD + 8, dt, dev, "nan").put(q)
    dod = Buf(total, HD, HD + 16, dt, dev, "nan").put(do)
    kv = Buf(N_IMG * Tk, 2 * HD, 2 * HD + 16, dt, dev, "nan").put(k).put(v, HD)
    kvr = Buf(B * Tk, 2 * HD, 2 * HD + 16, dt, dev, "nan").put(krep).put(vrep, HD)
    offd, lend = (torch.from_numpy(q_off).to(dev), torch.tensor(ql, dtype=torch.int32, device=dev)) if packed else (None, None)
    mk_out = lambda: (Buf(total, HD, HD + 8, dt, dev, "canary"),  # noqa: E731
                      Buf(1, B * H * Tm, B * H * Tm, torch.float32, dev, "canary", off=4, extra=0))
    ld = dict(ldq=qd.ld, ldk=kv.ld, ldv=kv.ld)

    # ---- forward
    out, lse = mk_out()
    f_bits = _twice(lambda: ops.attn_fwd_shared(qd.t, kv.cols_of(0, HD), kv.cols_of(HD, HD), out.t, N_IMG, G, H, Tm, Tk, ldo=out.ld,
                                                q_off=offd, q_len=lend, lse=lse.t, **ld), [out, lse], what + " fwd")
    out.check_canary(what + " out")
    lse_w = torch.zeros(B, H, Tm, dtype=torch.bool)
    for b, n in enumerate(ql):
        lse_w[b, :, :n] = True
    lse.check_canary(what + " lse (no slot behind q_len)", lse_w.reshape(1, -1))
    out2, lse2 = mk_out()
    if packed:
        ops.attn_fwd_packed(qd.t, kvr.cols_of(0, HD), kvr.cols_of(HD, HD), out2.t, B, H, Tm, Tk, offd, lend, kv_packed=0, ldo=out2.ld,
                            lse=lse2.t, **ld)
    else:
        ops.attn_fwd(qd.t, kvr.cols_of(0, HD), kvr.cols_of(HD, HD), out2.t, B, H, Tm, Tk, ldo=out2.ld, lse=lse2.t, **ld)
    torch.cuda.synchronize()
    assert torch.equal(out2.bits(), f_bits[0]), what + ": out differs from the one-tile kernel on replicated K / V"
    assert torch.equal(lse2.bits(), f_bits[1]), what + ": lse differs from the one-tile kernel on replicated K / V"

    # ---- backward
    dq = Buf(total, HD, HD + 24, dt, dev, "canary")
    dkv = Buf(N_IMG * Tk, 2 * HD, 2 * HD + 16, dt, dev, "canary")
    ldb = dict(ld, ldo=out.ld, lddo=dod.ld, lddq=dq.ld, lddk=dkv.ld, lddv=dkv.ld)
    b_bits = _twice(lambda: ops.attn_bwd_shared(qd.t, kv.cols_of(0, HD), kv.cols_of(HD, HD), out.t, dod.t, lse.t, dq.t, dkv.cols_of(0, HD),
                                                dkv.cols_of(HD, HD), N_IMG, G, H, Tm, Tk, q_off=offd, q_len=lend, **ldb), [dq, dkv],
                    what + " bwd")
    dq.check_canary(what + " dq")
    dkv.check_canary(what + " dk | dv")
    dq2 = Buf(total, HD, HD + 24, dt, dev, "canary")
    dkv2 = Buf(B * Tk, 2 * HD, 2 * HD + 16, dt, dev, "canary")
    args = (qd.t, kvr.cols_of(0, HD), kvr.cols_of(HD, HD), out.t, dod.t, lse.t, dq2.t, dkv2.cols_of(0, HD), dkv2.cols_of(HD, HD), B, H, Tm, Tk)
    if packed:
        ops.attn_bwd_packed(*args, offd, lend, kv_packed=0, **ldb)
    else:
        ops.attn_bwd(*args, **ldb)
    torch.cuda.synchronize()
    assert torch.equal(dq2.bits(), b_bits[0]), what + ": dq differs from the one-tile kernel on replicated K / V"
    if G == 1:
        assert torch.equal(dkv2.bits(), b_bits[1]), what + ": G = 1, dk / dv differ from the one-tile kernel"

    # ---- dk / dv against fp64, per caption, summed over an image's captions
    go, gl = out.get(), lse.get().reshape(B, H, Tm)
    gk, gv = dkv.get(0, HD), dkv.get(HD, HD)
    assert np.isfinite(gk).all() and np.isfinite(gv).all(), what
    for i in range(N_IMG):
        rk = slice(i * Tk, (i + 1) * Tk)
        ref = {n: 0.0 for n in ("dK", "dV", "bound_dK", "bound_dV")}
        for g in range(G):
            b = i * G + g
            r = slice(int(q_off[b]), int(q_off[b]) + ql[b])
            x = AR.bwd_ref(_hd(q[r]), _hd(k[rk]), _hd(v[rk]), _hd(do[r]), AR.allowed_mask(ql[b], Tk), dtype, out=_hd(go[r]),
                           lse=gl[b, :, :ql[b]])
            for n in ref:
                ref[n] = ref[n] + x[n]
        AR.check(_hd(gk[rk]), ref["dK"], ref["bound_dK"], f"shared/{dtype} dK: {what} image {i}")
        AR.check(_hd(gv[rk]), ref["dV"], ref["bound_dV"], f"shared/{dtype} dV: {what} image {i}")


def _refused(fn, outs, what):
    from mic_amd._lib import MicError

    for o in outs:
        o.refill()
    with pytest.raises(MicError):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        o.check_canary(what, torch.zeros(o.rows, o.cols, dtype=torch.bool))


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_refused_calls_write_nothing(dev, dtype):
    from mic_amd import ops

    dt, G, T = TD[dtype], 2, 65
    B = N_IMG * G
    odd = HD + (4 if dtype == "bf16" else 2)  # a row stride that is not a multiple of 16 B
    mk = lambda fill: Buf(B * T, HD, HD + 8, dt, dev, fill)  # noqa: E731
    q, k, v, do = (mk("nan").put(np.ones((B * T, HD))) for _ in range(4))
    out, dq, dk, dv = (mk("canary") for _ in range(4))
    lse = Buf(1, B * H * T, B * H * T, torch.float32, dev, "canary", off=4, extra=0)
    outs = [out, lse, dq, dk, dv]
    ld = dict(ldq=q.ld, ldk=k.ld, ldv=v.ld, ldo=out.ld)
    ldb = dict(ld, lddo=do.ld, lddq=dq.ld, lddk=dk.ld, lddv=dv.ld)
    fwd = lambda n, g, tq, tk, **kw: ops.attn_fwd_shared(q.t, k.t, v.t, out.t, n, g, H, tq, tk, lse=lse.t, **dict(ld, **kw))  # noqa: E731
    bwd = lambda n, g, tq, tk, **kw: ops.attn_bwd_shared(q.t, k.t, v.t, out.t, do.t, lse.t, dq.t, dk.t, dv.t, n, g, H, tq, tk,  # noqa: E731
                                                         **dict(ldb, **kw))
    for name, call in (("fwd", fwd), ("bwd", bwd)):
        _refused(lambda: call(N_IMG, G, 65, 64), outs, name + " Tq_max 65")
        _refused(lambda: call(N_IMG, G, 64, 65), outs, name + " Tk 65")
        _refused(lambda: call(N_IMG, 0, 64, 64), outs, name + " G 0")
        _refused(lambda: call(N_IMG, G, 64, 64, ldq=odd), outs, name + " ldq")
        _refused(lambda: call(N_IMG, G, 64, 64, ldk=odd), outs, name + " ldk")
    _refused(lambda: bwd(N_IMG, G, 64, 64, lddo=odd), outs, "bwd lddo")
    qlen = torch.tensor([64] * B, dtype=torch.int32, device=dev)
    _refused(lambda: fwd(N_IMG, G, 64, 64, q_off=None, q_len=qlen), outs, "q_len without q_off")
