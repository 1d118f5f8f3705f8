"""Attention conformance on the MI355X: every case of tests/util_attn_cases.py (the product's shapes, the ragged edges of the
single-tile and the tiled kernels, packed rows, the probs and decode kernels with every dispatch branch) in both storage types
against the fp64 reference and the derived per-element bounds of tests/util_attn_ref.py.  Around every call:
  - outputs (out, lse, dQ / dK / dV, probs, the caches of mic_kv_append) are windows inside larger allocations filled with a
    NaN-payload canary: extra rows behind, a row stride wider than the used columns, a base 16 B (bf16) / 32 B (fp32) into the
    allocation; every element outside the window — and lse[b][h][i], i >= q_len[b] — must keep its bits;
  - what a kernel must not read (rows past the operands, the padding inside the row stride, cache slots > cur, cache rows that
    no src_row entry names) holds NaN; masked keys and the neighbouring operands of a fused [rows][3d] / [rows][2d] buffer hold
    finite values of ordinary size (0 * NaN is NaN in the reference too: NaN there would prove nothing);
  - every path runs twice and must give identical bits (no attention kernel uses atomics).
The backward is checked twice: against its contract on the out / lse it was handed (the device forward's, as stored), and end to
end against the fp64 gradient of softmax(s) V."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_attn_cases as AC  # noqa: E402
import util_attn_ref as AR  # noqa: E402
import util_gemm_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu

TD = {"bf16": torch.bfloat16, "f32": torch.float32}
IB = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
D = 64


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
        """fp64 numpy [rows][n] -> columns [c0, c0 + n) of the window"""
        self.full[:self.rows, c0:c0 + x.shape[1]] = torch.from_numpy(np.ascontiguousarray(x)).to(self.flat.device).to(self.flat.dtype)
        return self

    def cols_of(self, c0, n):
        return self.full[:self.rows, c0:c0 + n]

    def get(self, c0=0, n=None):
        return self.full[:self.rows, c0:c0 + (self.cols - c0 if n is None else n)].double().cpu().numpy()

    def bits(self):
        return self.flat.view(IB[self.flat.dtype]).clone()

    def check_canary(self, what, written=None):
        """everything outside the window (and, with `written` [rows][cols] bool, outside its True part) kept its bits"""
        w = torch.zeros(self.flat.shape, dtype=torch.bool, device=self.flat.device)
        win = w[self.off:self.off + self.full.numel()].view(self.full.shape)[:self.rows, :self.cols]
        win[...] = True if written is None else written.to(w.device)
        AR.check_canary_mask(self.flat, w, what)


def _twice(run, outs, what):
    """run the launch twice from freshly canary-filled outputs: identical bits"""
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


def _heads(x, B, T, H):
    """[B*T][H*64] -> [B][H][T][64]"""
    return x.reshape(B, T, H, D).transpose(0, 2, 1, 3)


def _operands(layout, nq, nk, HD, dt, dev, q, k, v):
    """device operands in the layout's buffers: (q, k, v tensors, ldq, ldk, ldv)"""
    if layout == "fused3":
        assert nq == nk
        b = Buf(nq, 3 * HD, 3 * HD + 8, dt, dev, "nan").put(q).put(k, HD).put(v, 2 * HD)
        return b.cols_of(0, HD), b.cols_of(HD, HD), b.cols_of(2 * HD, HD), b.ld, b.ld, b.ld
    if layout == "kv2":
        bq = Buf(nq, HD, HD + 8, dt, dev, "nan").put(q)
        b = Buf(nk, 2 * HD, 2 * HD + 16, dt, dev, "nan").put(k).put(v, HD)
        return bq.t, b.cols_of(0, HD), b.cols_of(HD, HD), bq.ld, b.ld, b.ld
    bq, bk, bv = (Buf(n, HD, HD + p, dt, dev, "nan").put(x) for n, p, x in ((nq, 8, q), (nk, 16, k), (nk, 24, v)))
    return bq.t, bk.t, bv.t, bq.ld, bk.ld, bv.ld


def _grad_bufs(layout, nq, nk, HD, dt, dev):
    """(dq, dk, dv tensors, lddq, lddk, lddv, [Buf], getters)"""
    if layout == "fused3":
        b = Buf(nq, 3 * HD, 3 * HD + 8, dt, dev, "canary")
        return (b.cols_of(0, HD), b.cols_of(HD, HD), b.cols_of(2 * HD, HD), b.ld, b.ld, b.ld, [b],
                lambda: (b.get(0, HD), b.get(HD, HD), b.get(2 * HD, HD)))
    if layout == "kv2":
        bq, b = Buf(nq, HD, HD + 8, dt, dev, "canary"), Buf(nk, 2 * HD, 2 * HD + 16, dt, dev, "canary")
        return bq.t, b.cols_of(0, HD), b.cols_of(HD, HD), bq.ld, b.ld, b.ld, [bq, b], lambda: (bq.get(), b.get(0, HD), b.get(HD, HD))
    bq, bk, bv = (Buf(n, HD, HD + p, dt, dev, "canary") for n, p in ((nq, 24), (nk, 8), (nk, 16)))
    return bq.t, bk.t, bv.t, bq.ld, bk.ld, bv.ld, [bq, bk, bv], lambda: (bq.get(), bk.get(), bv.get())


def _sample_batches(B, name):
    if B <= 8:
        return np.arange(B)
    rng = np.random.default_rng(len(name))
    return np.array(sorted({0, 1, 2, B - 1} | set(rng.choice(B, 5, replace=False).tolist())))


def _check_problem(tag, case, dtype, q, k, v, do, allowed, got_out, got_lse, got_grads):
    """forward and both backward checks of [..., T, 64] problems"""
    f = AR.fwd_ref(q, k, v, allowed, dtype)
    AR.check(got_out, f["O"], f["bound_O"], f"{tag} out: {case}")
    AR.check_lse(got_lse, f["lse"], f["bound_lse"], f"{tag} lse: {case}")
    dead = np.isneginf(f["lse"])
    if dead.any():  # rows with no admissible key: zeros, exactly
        assert not got_out[dead].any(), f"{case}: out of a row with no admissible key is not 0"
    if got_grads is None:
        return
    b = AR.bwd_ref(q, k, v, do, allowed, dtype, out=got_out, lse=got_lse)
    e = AR.bwd_ref(q, k, v, do, allowed, dtype)
    for g, n in zip(got_grads, ("dQ", "dK", "dV")):
        assert np.isfinite(g).all(), f"{case}: {n} not finite"
        AR.check(g, b[n], b["bound_" + n], f"{tag} {n}: {case}")
        AR.check(g, e[n], e["bound_" + n], f"{tag} {n} end to end: {case}")
    if dead.any():
        assert not got_grads[0][dead].any(), f"{case}: dQ of a row with no admissible key is not 0"


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in AC.DENSE])
def test_attn_dense(dev, name, dtype):
    from mic_amd import ops

    c = AC.BY_NAME[name]
    B, H, Tq, Tk, HD, dt = c["B"], c["H"], c["Tq"], c["Tk"], c["H"] * D, TD[dtype]
    q, k, v, do, km = AC.dense_inputs(c, dtype)
    qd, kd, vd, ldq, ldk, ldv = _operands(c["layout"], B * Tq, B * Tk, HD, dt, dev, q, k, v)
    dod = Buf(B * Tq, HD, HD + 16, dt, dev, "nan").put(do)
    kmd = torch.from_numpy(km).to(dev) if km is not None else None
    out = Buf(B * Tq, HD, HD + 8, dt, dev, "canary")
    lse = Buf(1, B * H * Tq, B * H * Tq, torch.float32, dev, "canary", off=4, extra=0)
    kw = dict(ldq=ldq, ldk=ldk, ldv=ldv, ldo=out.ld, key_mask=kmd, causal=c["causal"])
    _twice(lambda: ops.attn_fwd(qd, kd, vd, out.t, B, H, Tq, Tk, lse=lse.t, **kw), [out, lse], name + " fwd")
    out.check_canary(name + " out")
    lse.check_canary(name + " lse")
    dq, dk, dv, lddq, lddk, lddv, gbufs, grads = _grad_bufs(c["layout"], B * Tq, B * Tk, HD, dt, dev)
    _twice(lambda: ops.attn_bwd(qd, kd, vd, out.t, dod.t, lse.t, dq, dk, dv, B, H, Tq, Tk, lddo=dod.ld, lddq=lddq, lddk=lddk,
                                lddv=lddv, **kw), gbufs, name + " bwd")
    for g in gbufs:
        g.check_canary(name + " gradients")
    bs = _sample_batches(B, name)
    allowed = AR.allowed_mask(Tq, Tk, c["causal"], km[bs][:, None, :] if km is not None else None)
    hq = lambda x, T: _heads(x, B, T, H)[bs]  # noqa: E731
    gq, gk, gv = grads()
    _check_problem(f"{c['claim']}/{dtype}", name, dtype, hq(q, Tq), hq(k, Tk), hq(v, Tk), hq(do, Tq), allowed, hq(out.get(), Tq),
                   lse.get().reshape(B, H, Tq)[bs], (hq(gq, Tq), hq(gk, Tk), hq(gv, Tk)))


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in AC.PACKED])
def test_attn_packed(dev, name, dtype):
    from mic_amd import ops

    c = AC.BY_NAME[name]
    B, H, Tm, Tk, HD, dt, ql = c["B"], c["H"], c["Tq_max"], c["Tk"], c["H"] * D, TD[dtype], c["q_len"]
    q, k, v, do, q_off = AC.packed_inputs(c, dtype)
    total, nk = q.shape[0], k.shape[0]
    qd, kd, vd, ldq, ldk, ldv = _operands(c["layout"], total, nk, HD, dt, dev, q, k, v)
    dod = Buf(total, HD, HD + 16, dt, dev, "nan").put(do)
    offd, lend = torch.from_numpy(q_off).to(dev), torch.tensor(ql, dtype=torch.int32, device=dev)
    out = Buf(total, HD, HD + 8, dt, dev, "canary")
    lse = Buf(1, B * H * Tm, B * H * Tm, torch.float32, dev, "canary", off=4, extra=0)
    kw = dict(kv_packed=c["kv_packed"], ldq=ldq, ldk=ldk, ldv=ldv, ldo=out.ld, causal=c["causal"])
    _twice(lambda: ops.attn_fwd_packed(qd, kd, vd, out.t, B, H, Tm, Tk, offd, lend, lse=lse.t, **kw), [out, lse], name + " fwd")
    out.check_canary(name + " out")
    lse_written = torch.zeros(B, H, Tm, dtype=torch.bool)
    for b, n in enumerate(ql):
        lse_written[b, :, :n] = True
    lse.check_canary(name + " lse (entries i >= q_len[b] are not written)", lse_written.reshape(1, -1))
    dq, dk, dv, lddq, lddk, lddv, gbufs, grads = _grad_bufs(c["layout"], total, nk, HD, dt, dev)
    _twice(lambda: ops.attn_bwd_packed(qd, kd, vd, out.t, dod.t, lse.t, dq, dk, dv, B, H, Tm, Tk, offd, lend, lddo=dod.ld, lddq=lddq,
                                       lddk=lddk, lddv=lddv, **kw), gbufs, name + " bwd")
    for g in gbufs:
        g.check_canary(name + " gradients")
    go, gl, (gq, gk, gv) = out.get(), lse.get().reshape(B, H, Tm), grads()
    hd = lambda x: x.reshape(x.shape[0], H, D).transpose(1, 0, 2)  # noqa: E731  [T][H*64] -> [H][T][64]
    for b, n in enumerate(ql):
        r = slice(int(q_off[b]), int(q_off[b]) + n)
        rk = r if c["kv_packed"] else slice(b * Tk, (b + 1) * Tk)
        allowed = AR.allowed_mask(n, rk.stop - rk.start, c["causal"])
        _check_problem(f"packed/{dtype}", f"{name} b={b}", dtype, hd(q[r]), hd(k[rk]), hd(v[rk]), hd(do[r]), allowed, hd(go[r]),
                       gl[b, :, :n], (hd(gq[r]), hd(gk[rk]), hd(gv[rk])))
    if c["dense_twin"]:  # every sequence full: the dense entry points on the same buffers give the same bits
        first = [t.bits() for t in [out, lse] + gbufs]
        for t in [out, lse] + gbufs:
            t.refill()
        dkw = dict(ldq=ldq, ldk=ldk, ldv=ldv, ldo=out.ld, causal=c["causal"])
        ops.attn_fwd(qd, kd, vd, out.t, B, H, Tm, Tk, lse=lse.t, **dkw)
        ops.attn_bwd(qd, kd, vd, out.t, dod.t, lse.t, dq, dk, dv, B, H, Tm, Tk, lddo=dod.ld, lddq=lddq, lddk=lddk, lddv=lddv, **dkw)
        torch.cuda.synchronize()
        for t, f in zip([out, lse] + gbufs, first):
            assert torch.equal(t.bits(), f), f"{name}: packed and dense differ"


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in AC.PROBS])
def test_attn_probs(dev, name, dtype):
    from mic_amd import ops

    c = AC.BY_NAME[name]
    B, H, Tq, Tk, HD, dt = c["B"], c["H"], c["Tq"], c["Tk"], c["H"] * D, TD[dtype]
    q, k, _, _, km = AC.dense_inputs(dict(c, qscale=1.0, dominant=True, shift=False), dtype)
    qd, kd, _, ldq, ldk, _ = _operands("kv2", B * Tq, B * Tk, HD, dt, dev, q, k, k)
    kmd = torch.from_numpy(km).to(dev) if km is not None else None
    n = B * H * Tq * Tk
    out = Buf(1, n, n, torch.float32, dev, "canary", off=4, extra=0)
    _twice(lambda: ops.attn_probs(qd, kd, out.t, B, H, Tq, Tk, ldq=ldq, ldk=ldk, key_mask=kmd, causal=c["causal"]), [out], name)
    out.check_canary(name)
    allowed = AR.allowed_mask(Tq, Tk, c["causal"], km[:, None, :] if km is not None else None)
    f = AR.fwd_ref(_heads(q, B, Tq, H), _heads(k, B, Tk, H), _heads(k, B, Tk, H), allowed, dtype, u_p=AR.U32)
    got = out.get().reshape(B, H, Tq, Tk)
    AR.check(got, f["P"], f["bound_P"], f"probs/{dtype} P: {name}")
    assert not got[~np.broadcast_to(allowed, got.shape)].any(), f"{name}: a disallowed pair is not exactly 0"


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in AC.DECODE])
def test_attn_decode(dev, name, dtype):
    from mic_amd import ops

    c = AC.BY_NAME[name]
    R, H, L, cur, HD, dt = c["R"], c["H"], c["max_len"], c["cur"], c["H"] * D, TD[dtype]
    q, kc, vc, src = AC.decode_inputs(c, dtype)
    rows = kc.shape[0]
    qd = Buf(R, HD, HD + 8, dt, dev, "nan").put(q)
    if c["ldc2"]:  # k and v are the halves of one fused projection: slots of 2 HD elements
        cache = Buf(rows * L, 2 * HD, 2 * HD, dt, dev, "nan", extra=0).put(kc.reshape(rows * L, HD)).put(vc.reshape(rows * L, HD), HD)
        kcd, vcd, ldc = cache.cols_of(0, HD), cache.cols_of(HD, HD), 2 * HD
    else:
        kb, vb = (Buf(rows * L, HD, HD, dt, dev, "nan", extra=0).put(x.reshape(rows * L, HD)) for x in (kc, vc))
        kcd, vcd, ldc = kb.t, vb.t, HD
    srcd = torch.from_numpy(src).to(dev) if src is not None else None
    out = Buf(R, HD, HD + 8, dt, dev, "canary")
    _twice(lambda: ops.attn_decode(qd.t, kcd, vcd, out.t, R, H, L, cur, ldq=qd.ld, ldo=out.ld, ldc=ldc, src_row=srcd,
                                   row_div=c["row_div"]), [out], name)
    out.check_canary(name)
    ref, bound = AR.decode_ref(q, kc, vc, H, L, cur, dtype, src_row=src, row_div=c["row_div"])
    AR.check(out.get(), ref, bound, f"decode_{c['claim']}/{dtype} out: {name}")


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("R,HD,L,cur", AC.KV_APPEND)
def test_kv_append(dev, dtype, R, HD, L, cur):
    """a bit-exact copy into slot `cur` of every row's cache; every other slot of both caches keeps its canary"""
    from mic_amd import ops

    dt = TD[dtype]
    rng = np.random.default_rng(R * L + cur)
    k, v = (GR.round_to(rng.standard_normal((R, HD)), dtype) for _ in range(2))
    src = Buf(R, 2 * HD, 2 * HD + 8, dt, dev, "nan").put(k).put(v, HD)
    kc, vc = (Buf(R * L, HD, HD, dt, dev, "canary") for _ in range(2))
    _twice(lambda: ops.kv_append(src.cols_of(0, HD), src.cols_of(HD, HD), kc.t, vc.t, R, HD, L, cur, ldk=src.ld, ldv=src.ld), [kc, vc],
           "kv_append")
    written = torch.zeros(R, L, HD, dtype=torch.bool)
    written[:, cur] = True
    for cache, x, what in ((kc, k, "k cache"), (vc, v, "v cache")):
        cache.check_canary(what, written.reshape(R * L, HD))
        assert np.array_equal(cache.get().reshape(R, L, HD)[:, cur], x), what


def _refused(fn, outs, what):
    """MicError on the host, before any launch: the outputs keep every canary"""
    from mic_amd._lib import MicError

    for o in outs:
        o.refill()
    with pytest.raises(MicError):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        o.check_canary(what, torch.zeros(o.rows, o.cols, dtype=torch.bool))


@pytest.mark.parametrize("dtype", AC.DTYPES)
def test_attn_refusals(dev, dtype):
    from mic_amd import _lib as L
    from mic_amd import ops

    dt, H, HD, B, T = TD[dtype], 2, 128, 2, 65
    odd = HD + (4 if dtype == "bf16" else 2)  # a row stride that is not a multiple of 16 B
    mk = lambda fill, rows=B * T, cols=HD, ld=HD + 8: Buf(rows, cols, ld, dt, dev, fill)  # noqa: E731
    q, k, v, do = (mk("nan").put(np.ones((B * T, HD))) for _ in range(4))
    out, dq, dk, dv = (mk("canary") for _ in range(4))
    lse = Buf(1, B * H * T, B * H * T, torch.float32, dev, "canary", off=4, extra=0)
    qo, qlen = torch.tensor([0, 64], dtype=torch.int32, device=dev), torch.tensor([64, 64], dtype=torch.int32, device=dev)
    ld = dict(ldq=q.ld, ldk=k.ld, ldv=v.ld, ldo=out.ld)
    ldb = dict(ld, lddo=do.ld, lddq=dq.ld, lddk=dk.ld, lddv=dv.ld)
    outs = [out, lse, dq, dk, dv]
    # packed: one 64x64 tile per sequence
    _refused(lambda: ops.attn_fwd_packed(q.t, k.t, v.t, out.t, B, H, 65, 64, qo, qlen, kv_packed=0, lse=lse.t, **ld), outs, "Tq_max 65")
    _refused(lambda: ops.attn_fwd_packed(q.t, k.t, v.t, out.t, B, H, 64, 65, qo, qlen, kv_packed=0, lse=lse.t, **ld), outs, "Tk 65")
    _refused(lambda: ops.attn_bwd_packed(q.t, k.t, v.t, out.t, do.t, lse.t, dq.t, dk.t, dv.t, B, H, 65, 64, qo, qlen, kv_packed=0, **ldb),
             outs, "bwd Tq_max 65")
    _refused(lambda: ops.attn_bwd_packed(q.t, k.t, v.t, out.t, do.t, lse.t, dq.t, dk.t, dv.t, B, H, 64, 65, qo, qlen, kv_packed=0, **ldb),
             outs, "bwd Tk 65")
    _refused(lambda: ops.attn_fwd_packed(q.t, k.t, v.t, out.t, B, H, 64, 64, None, qlen, kv_packed=0, lse=lse.t, **ld), outs, "q_off NULL")
    # a row stride that breaks the 16-B alignment of the staged rows (single tile and tiled)
    for Tq in (64, 65):
        _refused(lambda: ops.attn_fwd(q.t, k.t, v.t, out.t, B, H, Tq, Tq, lse=lse.t, **dict(ld, ldk=odd)), outs, "ldk")
        _refused(lambda: ops.attn_bwd(q.t, k.t, v.t, out.t, do.t, lse.t, dq.t, dk.t, dv.t, B, H, Tq, Tq, **dict(ldb, lddo=odd)), outs, "lddo")
        # a null operand, a storage type the library does not know
        _refused(lambda: ops.attn_fwd(q.t, None, v.t, out.t, B, H, Tq, Tq, lse=lse.t, **ld), outs, "k NULL")
        _refused(lambda: ops.attn_bwd(q.t, k.t, v.t, out.t, do.t, None, dq.t, dk.t, dv.t, B, H, Tq, Tq, **ldb), outs, "lse NULL")
        _refused(lambda: L.check(L.lib().mic_attn_fwd(7, B, H, Tq, Tq, q.t.data_ptr(), q.ld, k.t.data_ptr(), k.ld, v.t.data_ptr(), v.ld,
                                                      out.t.data_ptr(), out.ld, None, 0, lse.t.data_ptr(), None)), outs, "dtype 7")
    _refused(lambda: ops.attn_fwd(q.t.to(torch.float16), k.t, v.t, out.t, B, H, 64, 64, lse=lse.t, **ld), outs, "fp16")
    # probs: at most 1024 keys
    pr = Buf(1, 2 * 1025, 2 * 1025, torch.float32, dev, "canary", off=4, extra=0)
    kk = Buf(1025, HD, HD + 8, dt, dev, "nan").put(np.ones((1025, HD)))
    _refused(lambda: ops.attn_probs(q.t, kk.t, pr.t, 1, H, 1, 1025, ldq=q.ld, ldk=kk.ld), [pr], "probs Tk 1025")
    # decode / kv_append
    R, Lc = 4, 8
    kc, vc = (Buf(R * Lc, HD, HD, dt, dev, "canary") for _ in range(2))
    _refused(lambda: ops.kv_append(q.t, k.t, kc.t, vc.t, R, HD, Lc, Lc, ldk=q.ld, ldv=k.ld), [kc, vc], "kv_append cur = max_len")
    _refused(lambda: ops.kv_append(q.t, None, kc.t, vc.t, R, HD, Lc, 0, ldk=q.ld, ldv=k.ld), [kc, vc], "kv_append v NULL")
    kc.put(np.ones((R * Lc, HD)))
    vc.put(np.ones((R * Lc, HD)))
    _refused(lambda: ops.attn_decode(q.t, kc.t, vc.t, out.t, R, H, Lc, 3, ldq=odd, ldo=out.ld), [out], "decode ldq")
    _refused(lambda: ops.attn_decode(q.t, kc.t, None, out.t, R, H, Lc, 3, ldq=q.ld, ldo=out.ld), [out], "decode vc NULL")
    _refused(lambda: ops.attn_decode(q.t, kc.t, vc.t, out.t, R, H, Lc, -1, ldq=q.ld, ldo=out.ld), [out], "decode cur < 0")
