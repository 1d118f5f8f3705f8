"""Packed rows through the tiled attention kernels (ops.attn_fwd_packed_tiled / attn_bwd_packed_tiled) on the MI355X: every case of
tests/util_attn_packed_tiled_cases.py in both storage types against the fp64 reference and the derived per-element bounds of
tests/util_attn_ref.py — the checker, the buffers and the two backward checks are those of tests/test_attn_conformance_gpu.py
(test_attn_packed and the dense `tiled` cases), no tolerance of its own.  Around every call, as there: outputs are windows inside
canary-filled allocations (rows behind the packed total, a row stride wider than the used columns, lse slots i >= q_len[b] must keep
their bits), operands the kernels must not read hold NaN, and every launch runs twice with identical bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_attn_conformance_gpu as C  # noqa: E402  (Buf, _twice, _operands, _grad_bufs, _check_problem, _sample_batches, _refused)
import util_attn_packed_tiled_cases as PC  # noqa: E402
import util_attn_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu

TD, D = C.TD, C.D


def _run(dev, c, dtype, sample=None):
    """forward + backward of one case, canaries and the reference on the sequences `sample` (None: all); returns what a dense twin
    needs: (operands, outputs, launch keywords)"""
    from mic_amd import ops

    name = c["name"]
    B, H, Tm, Tk, HD, dt, ql = c["B"], c["H"], c["Tq_max"], c["Tk"], c["H"] * D, TD[dtype], c["q_len"]
    q, k, v, do, q_off = PC.packed_inputs(c, dtype)
    total, nk = q.shape[0], k.shape[0]
    qd, kd, vd, ldq, ldk, ldv = C._operands(c["layout"], total, nk, HD, dt, dev, q, k, v)
    dod = C.Buf(total, HD, HD + 16, dt, dev, "nan").put(do)
    offd, lend = torch.from_numpy(q_off).to(dev), torch.tensor(ql, dtype=torch.int32, device=dev)
    out = C.Buf(total, HD, HD + 8, dt, dev, "canary")
    lse = C.Buf(1, B * H * Tm, B * H * Tm, torch.float32, dev, "canary", off=4, extra=0)
    kw = dict(kv_packed=c["kv_packed"], ldq=ldq, ldk=ldk, ldv=ldv, ldo=out.ld, causal=c["causal"])
    C._twice(lambda: ops.attn_fwd_packed_tiled(qd, kd, vd, out.t, B, H, Tm, Tk, offd, lend, lse=lse.t, **kw), [out, lse], name + " fwd")
    out.check_canary(name + " out")
    lse_written = torch.zeros(B, H, Tm, dtype=torch.bool)
    for b, n in enumerate(ql):
        lse_written[b, :, :n] = True
    lse.check_canary(name + " lse (entries i >= q_len[b] are not written)", lse_written.reshape(1, -1))
    dq, dk, dv, lddq, lddk, lddv, gbufs, grads = C._grad_bufs(c["layout"], total, nk, HD, dt, dev)
    C._twice(lambda: ops.attn_bwd_packed_tiled(qd, kd, vd, out.t, dod.t, lse.t, dq, dk, dv, B, H, Tm, Tk, offd, lend, lddo=dod.ld,
                                               lddq=lddq, lddk=lddk, lddv=lddv, **kw), gbufs, name + " bwd")
    for g in gbufs:
        g.check_canary(name + " gradients")
    go, gl, (gq, gk, gv) = out.get(), lse.get().reshape(B, H, Tm), grads()
    hd = lambda x: x.reshape(x.shape[0], H, D).transpose(1, 0, 2)  # noqa: E731  [T][H*64] -> [H][T][64]
    for b in (range(B) if sample is None else sample):
        n = ql[b]
        r = slice(int(q_off[b]), int(q_off[b]) + n)
        rk = r if c["kv_packed"] else slice(b * Tk, (b + 1) * Tk)
        allowed = AR.allowed_mask(n, rk.stop - rk.start, c["causal"])
        C._check_problem(f"packed_tiled/{dtype}", f"{name} b={b}", dtype, hd(q[r]), hd(k[rk]), hd(v[rk]), hd(do[r]), allowed, hd(go[r]),
                         gl[b, :, :n], (hd(gq[r]), hd(gk[rk]), hd(gv[rk])))
    return (qd, kd, vd, dod), (out, lse, gbufs, dq, dk, dv), dict(ldq=ldq, ldk=ldk, ldv=ldv, lddq=lddq, lddk=lddk, lddv=lddv)


@pytest.mark.parametrize("dtype", PC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in PC.SELF + PC.CROSS])
def test_attn_packed_tiled(dev, name, dtype):
    _run(dev, PC.BY_NAME[name], dtype)


@pytest.mark.parametrize("dtype", PC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in PC.TWINS])
def test_attn_packed_tiled_dense_twin(dev, name, dtype):
    """every sequence full: out, lse, dq, dk and dv are bit for bit what mic_attn_fwd / mic_attn_bwd give on the same rows (causal
    without a key mask for self-attention, not causal for cross-attention)"""
    from mic_amd import ops

    c = PC.BY_NAME[name]
    B, H, Tm, Tk = c["B"], c["H"], c["Tq_max"], c["Tk"]
    (qd, kd, vd, dod), (out, lse, gbufs, dq, dk, dv), ld = _run(dev, c, dtype)
    bufs = [out, lse] + gbufs
    first = [t.bits() for t in bufs]
    for t in bufs:
        t.refill()
    dkw = dict(ldq=ld["ldq"], ldk=ld["ldk"], ldv=ld["ldv"], ldo=out.ld, causal=c["causal"])
    ops.attn_fwd(qd, kd, vd, out.t, B, H, Tm, Tk, lse=lse.t, **dkw)
    ops.attn_bwd(qd, kd, vd, out.t, dod.t, lse.t, dq, dk, dv, B, H, Tm, Tk, lddo=dod.ld, lddq=ld["lddq"], lddk=ld["lddk"],
                 lddv=ld["lddv"], **dkw)
    torch.cuda.synchronize()
    for t, f in zip(bufs, first):
        assert torch.equal(t.bits(), f), f"{name}: packed and dense differ"


@pytest.mark.parametrize("dtype", PC.DTYPES)
@pytest.mark.parametrize("kind", ["self", "cross"])
def test_attn_packed_tiled_product_sized_launch(dev, kind, dtype):
    """B 64, H 16, Tq_max 128 on the caption lengths of a benchmark batch (2048 query-block workgroups, about half of them without
    work); the reference on a sample of the sequences, canaries and repeatability on all of them"""
    c = PC.product_case(kind)
    _run(dev, c, dtype, sample=C._sample_batches(c["B"], c["name"]))


@pytest.mark.parametrize("dtype", PC.DTYPES)
def test_attn_packed_tiled_refusals(dev, dtype):
    """refused on the host, before any launch, every output keeping its canary: NULL q_off / q_len, a row stride that breaks the
    16-B alignment, kv_packed with Tk != Tq_max, a storage type the library does not know"""
    from mic_amd import _lib as L
    from mic_amd import ops

    dt, H, HD, B, T = TD[dtype], 2, 128, 2, 65
    odd = HD + (4 if dtype == "bf16" else 2)  # a row stride that is not a multiple of 16 B
    mk = lambda fill: C.Buf(B * T, HD, HD + 8, dt, dev, fill)  # noqa: E731
    q, k, v, do = (mk("nan").put(np.ones((B * T, HD))) for _ in range(4))
    out, dq, dk, dv = (mk("canary") for _ in range(4))
    lse = C.Buf(1, B * H * T, B * H * T, torch.float32, dev, "canary", off=4, extra=0)
    qo, qlen = torch.tensor([0, 65], dtype=torch.int32, device=dev), torch.tensor([65, 65], dtype=torch.int32, device=dev)
    ld = dict(ldq=q.ld, ldk=k.ld, ldv=v.ld, ldo=out.ld)
    ldb = dict(ld, lddo=do.ld, lddq=dq.ld, lddk=dk.ld, lddv=dv.ld)
    outs = [out, lse, dq, dk, dv]
    fwd = lambda off=qo, ln=qlen, Tk=T, kvp=1, **o: ops.attn_fwd_packed_tiled(  # noqa: E731
        q.t, k.t, v.t, out.t, B, H, T, Tk, off, ln, kv_packed=kvp, lse=lse.t, **dict(ld, **o))
    bwd = lambda off=qo, ln=qlen, Tk=T, kvp=1, **o: ops.attn_bwd_packed_tiled(  # noqa: E731
        q.t, k.t, v.t, out.t, do.t, lse.t, dq.t, dk.t, dv.t, B, H, T, Tk, off, ln, kv_packed=kvp, **dict(ldb, **o))
    for call, what in ((fwd, "fwd"), (bwd, "bwd")):
        C._refused(lambda: call(off=None), outs, what + " q_off NULL")
        C._refused(lambda: call(ln=None), outs, what + " q_len NULL")
        for s in ("ldq", "ldk", "ldv"):
            C._refused(lambda: call(**{s: odd}), outs, f"{what} {s}")
        C._refused(lambda: call(Tk=64), outs, what + " kv_packed with Tk != Tq_max")
        C._refused(lambda: call(Tk=130), outs, what + " kv_packed with Tk != Tq_max")
    C._refused(lambda: bwd(ldo=odd), outs, "bwd ldo")
    C._refused(lambda: bwd(lddo=odd), outs, "bwd lddo")
    p = lambda t: t.t.data_ptr()  # noqa: E731
    C._refused(lambda: L.check(L.lib().mic_attn_fwd_packed_tiled(7, B, H, T, T, qo.data_ptr(), qlen.data_ptr(), 1, p(q), q.ld, p(k), k.ld,
                                                                 p(v), v.ld, p(out), out.ld, 1, p(lse), None)), outs, "fwd dtype 7")
    C._refused(lambda: L.check(L.lib().mic_attn_bwd_packed_tiled(7, B, H, T, T, qo.data_ptr(), qlen.data_ptr(), 1, p(q), q.ld, p(k), k.ld,
                                                                 p(v), v.ld, p(out), out.ld, p(do), do.ld, p(lse), 1, p(dq), dq.ld,
                                                                 p(dk), dk.ld, p(dv), dv.ld, None)), outs, "bwd dtype 7")
    C._refused(lambda: ops.attn_fwd_packed_tiled(q.t.to(torch.float16), k.t, v.t, out.t, B, H, T, T, qo, qlen, kv_packed=1, lse=lse.t, **ld),
               outs, "fp16")
    # the one-tile packed entry points keep their limit
    C._refused(lambda: ops.attn_fwd_packed(q.t, k.t, v.t, out.t, B, H, T, T, qo, qlen, kv_packed=1, lse=lse.t, **ld), outs, "one-tile Tq_max 65")
