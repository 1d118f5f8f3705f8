"""fp64 reference of the attention contract (include/mic_hip.h: mic_attn_fwd / bwd, the packed forms, mic_attn_probs,
mic_attn_decode) with per-element error bounds, and numpy emulations of the kernels' arithmetic for the suite's own checks
(tests/test_attn_conformance_{cpu,gpu}.py).  A helper module, not a conftest.  The checker, the bf16 rounding and the canaries are
those of tests/util_gemm_ref.py.

One problem = one (batch, head): q [Tq][64], k, v [Tk][64] (the values as stored, lifted to fp64) and `allowed` [Tq][Tk]
(causal: j <= i; key_mask[b][j] != 0; j < Tk).  Every function takes leading batch dimensions.

    s   = q.k / 8 over allowed pairs                     e_s = gamma_64 (|q|.|k|) / 8        (64 exact products, fp32 adds)
    P   = softmax(s),  O = P V,  lse = logsumexp(s)
    a row with no allowed key:  P = 0, O = 0, lse = -inf, exactly; it adds nothing to dQ / dK / dV

u = unit roundoff of the storage type (2^-8 bf16, 2^-24 fp32), u32 = 2^-24, gamma_n = 2 n u32, eps_f = 32 u32 (fp32 exp / log /
division), u_p = roundoff of the P / dS tiles as the second contraction consumes them: u for the tile kernels (bf16 tiles in LDS),
u32 for the decode and probs kernels (p stays in registers).  M_i = max over allowed j of e_s[i][j].

forward   p~_j = exp(s_j - m) carries (2 M + eps_f) relative (the score's own error and the row maximum's), the row sum the same
          plus gamma_Tk, the tile rounding u_p per product, the fp32 P V accumulation gamma_Tk, the stored result u:
              bound_O   = u |O| + (1 + u) [ (u_p + gamma_Tk) P|V| + (2 M + eps_f) (P|V| + |O|) ]
              bound_lse = M + u32 (|lse| + 1) + eps_f + gamma_Tk
probs         bound_P   = P (2 M + eps_f + gamma_Tk) + u32 P;  disallowed pairs are exact zeros
backward  on the inputs the entry point is given (out and lse AS STORED):
              P = exp(s - lse),  dp = dO V^T,  delta = sum_d dO out,  dS = P (dp - delta) / 8,  dQ = dS K,  dK = dS^T Q,  dV = P^T dO
              e_P     = P (e_s + u32 |lse| + eps_f (1 + |s - lse|))
              e_dp    = gamma_64 |dO||V|^T,   e_delta = gamma_64 sum |dO||out|
              e_dS    = (e_P |dp - delta| + P (e_dp + e_delta)) / 8 + 3 u32 |dS|
              t_P = e_P + u_p P,  t_dS = e_dS + u_p |dS|                                     (the tiles as consumed)
              bound_dQ = u |dQ| + (1 + u) (t_dS |K| + gamma_Tk |dS||K|)
              bound_dK = u |dK| + (1 + u) (t_dS^T |Q| + gamma_Tq |dS|^T |Q|)
              bound_dV = u |dV| + (1 + u) (t_P^T |dO| + gamma_Tq P^T |dO|)
end to end (forward then backward on the device, against the fp64 gradient of softmax(s) V from q, k, v alone): the backward reads
          the device's own out and lse, which differ from the exact ones by bound_O and bound_lse, so
              e_delta = gamma_64 sum |dO| (|O| + bound_O) + sum |dO| bound_O
              e_P     = the above + P bound_lse
          and everything downstream follows the same formulas.
decode    forward with u_p = u32 over the gathered slots 0 .. min(cur + 1, max_len) - 1.

Terms added after the first GPU run: none (see profiles/attn_conformance_worst_ratio.txt).
"""
from __future__ import annotations

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_gemm_ref as GR  # noqa: E402

U32 = GR.U32
EPS_F = GR.EPS_F
D = 64
gamma = GR.gamma_k
u_of = GR.u_of


def allowed_mask(Tq, Tk, causal=False, key_mask=None):
    """[..., Tq, Tk] bool; key_mask [..., Tk] (1 = attend) or None"""
    a = np.ones((Tq, Tk), bool)
    if causal:
        a &= np.arange(Tk)[None, :] <= np.arange(Tq)[:, None]
    if key_mask is not None:
        a = a & (np.asarray(key_mask) != 0)[..., None, :]
    return a


def _T(x):
    return np.swapaxes(x, -1, -2)


def _scores(q, k, allowed):
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    allowed = np.broadcast_to(allowed, q.shape[:-2] + (q.shape[-2], k.shape[-2]))
    s = q @ _T(k) / 8.0
    e_s = gamma(D) * (np.abs(q) @ _T(np.abs(k))) / 8.0
    return np.where(allowed, s, -np.inf), np.where(allowed, e_s, 0.0), allowed


def _softmax(s):
    m = s.max(-1, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0.0)
    p = np.exp(s - ms)
    l = p.sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(l > 0, p / np.where(l > 0, l, 1.0), 0.0)
        lse = np.where(l[..., 0] > 0, ms[..., 0] + np.log(l[..., 0]), -np.inf)
    return P, lse


def fwd_ref(q, k, v, allowed, dtype, u_p=None):
    """O, lse, P of the forward and their bounds"""
    u = u_of(dtype)
    u_p = u if u_p is None else u_p
    v = np.asarray(v, np.float64)
    s, e_s, allowed = _scores(q, k, allowed)
    Tk = s.shape[-1]
    P, lse = _softmax(s)
    O = P @ v
    PV = P @ np.abs(v)
    M = e_s.max(-1, keepdims=True)
    live = np.isfinite(lse)
    bound_O = u * np.abs(O) + (1 + u) * ((u_p + gamma(Tk)) * PV + (2 * M + EPS_F) * (PV + np.abs(O)))
    bound_lse = np.where(live, M[..., 0] + U32 * (np.abs(np.where(live, lse, 0.0)) + 1) + EPS_F + gamma(Tk), 0.0)
    bound_P = P * (2 * M + EPS_F + gamma(Tk)) + U32 * P
    return dict(O=O, lse=lse, P=P, bound_O=bound_O, bound_lse=bound_lse, bound_P=bound_P)


def bwd_ref(q, k, v, dout, allowed, dtype, *, out=None, lse=None, u_p=None):
    """dQ, dK, dV and their bounds.  With `out` and `lse` (as stored by the forward): the backward's contract on the inputs it is
    given.  Without: the gradient of softmax(s) V from q, k, v alone, the bound widened by what a device forward's stored out and
    lse add (module docstring)."""
    u = u_of(dtype)
    u_p = u if u_p is None else u_p
    q, k, v, dout = (np.asarray(t, np.float64) for t in (q, k, v, dout))
    s, e_s, allowed = _scores(q, k, allowed)
    Tq, Tk = s.shape[-2:]
    if out is None:
        f = fwd_ref(q, k, v, allowed, dtype, u_p)
        out, lse, d_out, d_lse = f["O"], f["lse"], f["bound_O"], f["bound_lse"]
    else:
        out, lse = np.asarray(out, np.float64), np.asarray(lse, np.float64)
        d_out, d_lse = np.zeros_like(out), np.zeros_like(lse)
    live = np.isfinite(lse)[..., None]
    lse_f = np.where(live, lse[..., None], 0.0)
    ok = allowed & live
    x = np.where(ok, s - lse_f, 0.0)
    P = np.where(ok, np.exp(x), 0.0)
    dp = dout @ _T(v)
    delta = (dout * out).sum(-1, keepdims=True)
    dS = P * (dp - delta) / 8.0
    e_P = P * (e_s + U32 * np.abs(lse_f) + EPS_F * (1 + np.abs(x)) + d_lse[..., None])
    e_dp = gamma(D) * (np.abs(dout) @ _T(np.abs(v)))
    e_delta = (gamma(D) * (np.abs(dout) * (np.abs(out) + d_out)).sum(-1, keepdims=True) + (np.abs(dout) * d_out).sum(-1, keepdims=True))
    e_dS = (e_P * np.abs(dp - delta) + P * (e_dp + e_delta)) / 8.0 + 3 * U32 * np.abs(dS)
    t_P = e_P + u_p * P
    t_dS = e_dS + u_p * np.abs(dS)
    dQ, dK, dV = dS @ k, _T(dS) @ q, _T(P) @ dout
    aK, aQ, aO = np.abs(k), np.abs(q), np.abs(dout)
    return dict(dQ=dQ, dK=dK, dV=dV, P=P, dS=dS,
                bound_dQ=u * np.abs(dQ) + (1 + u) * (t_dS @ aK + gamma(Tk) * (np.abs(dS) @ aK)),
                bound_dK=u * np.abs(dK) + (1 + u) * (_T(t_dS) @ aQ + gamma(Tq) * (_T(np.abs(dS)) @ aQ)),
                bound_dV=u * np.abs(dV) + (1 + u) * (_T(t_P) @ aO + gamma(Tq) * (_T(P) @ aO)))


def decode_ref(q, kc, vc, H, max_len, cur, dtype, *, src_row=None, row_div=1):
    """q [R][H*64]; kc, vc [rows][max_len][H*64] (fp64 of the stored values); -> (O [R][H*64], bound)"""
    q = np.asarray(q, np.float64)
    R = q.shape[0]
    n = min(cur + 1, max_len)
    slots = np.arange(n)
    rows = np.asarray(src_row)[:, :n] if src_row is not None else np.repeat((np.arange(R) // row_div)[:, None], n, 1)
    kk = np.asarray(kc, np.float64)[rows, slots[None, :]].reshape(R, n, H, D).transpose(0, 2, 1, 3)   # [R][H][n][64]
    vv = np.asarray(vc, np.float64)[rows, slots[None, :]].reshape(R, n, H, D).transpose(0, 2, 1, 3)
    f = fwd_ref(q.reshape(R, H, 1, D), kk, vv, np.ones((1, n), bool), dtype, u_p=U32)
    return f["O"].reshape(R, H * D), f["bound_O"].reshape(R, H * D)


def check(got, ref, bound, what, worst=None):
    """GR.check, keeping the worst ratio per `what` in the dict `worst`"""
    w = GR.check(got, ref, bound, what)
    if worst is not None:
        key = what.split(":")[0]
        worst[key] = max(worst.get(key, 0.0), w)
    return w


def check_lse(got, ref, bound, what, worst=None):
    """lse: -inf exactly where the reference row has no allowed key, within the bound elsewhere"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    dead = np.isneginf(ref)
    if not np.array_equal(np.isneginf(got), dead):
        i = np.argwhere(np.isneginf(got) != dead)[0]
        raise AssertionError(f"{what}: -inf pattern differs at {tuple(i)}: got {got[tuple(i)]!r} ref {ref[tuple(i)]!r}")
    return check(np.where(dead, 0.0, got), np.where(dead, 0.0, ref), bound, what, worst)


def check_canary_mask(t, written, what):
    """every element of the torch allocation `t` where the bool tensor `written` (same shape) is False still holds the canary"""
    import torch

    c = t.clone()
    iv = {torch.bfloat16: (torch.int16, GR.SENTINEL_BF16), torch.float32: (torch.int32, GR.SENTINEL_F32)}[t.dtype]
    c.view(iv[0])[written] = iv[1]
    GR.check_canary(c, None, what)


def old_criterion(got, ref):
    """the measure of tests/test_ops_gpu.py: max |err| / max |ref| over the whole tensor"""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------------------------------------------------------------------
# numpy emulations of the kernels' arithmetic (fp32 everywhere, the P / dS tiles and the results rounded to the storage type).
# `defect` seeds the mistakes the suite has to reject; None = the arithmetic as designed.
def _r(x, dtype):
    return GR.round_to(x, dtype).astype(np.float32)


def _f32(*ts):
    return [np.asarray(t, np.float64).astype(np.float32) for t in ts]


def emu_fwd(q, k, v, allowed, dtype, *, block=None, defect=None):
    """single problem (2-D operands).  block=None: the single-tile kernel (Tq, Tk <= 64; the tile is zero padded to 64 keys);
    block=64: the online-softmax walk over 64-key blocks.  Returns (out, lse) as fp64 of the stored values.
    defects: 'pad_key_in_sum' (one zero-padded key row counted in the row sum), 'no_alpha' (the rescale skipped when the running
    maximum moves in a later block)."""
    q, k, v = _f32(q, k, v)
    Tq, Tk = q.shape[0], k.shape[0]
    blk = block or max(Tk, 1)
    m_run = np.full(Tq, -np.inf, np.float32)
    l_run = np.zeros(Tq, np.float32)
    o = np.zeros((Tq, D), np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k0 in range(0, Tk, blk):
            kb, vb, ab = k[k0:k0 + blk], v[k0:k0 + blk], allowed[:, k0:k0 + blk]
            s = np.where(ab, (q @ kb.T) * np.float32(0.125), np.float32(-np.inf)).astype(np.float32)
            m_new = np.maximum(m_run, s.max(1))
            m_safe = np.where(np.isneginf(m_new), np.float32(0), m_new)
            p = np.exp(s - m_safe[:, None]).astype(np.float32)
            l = p.sum(1, dtype=np.float32)
            if defect == "pad_key_in_sum" and k0 + blk >= Tk:
                l = l + np.exp(-m_safe).astype(np.float32)  # the padded key's score is q.0 = 0
            alpha = np.where(np.isneginf(m_run), np.float32(0), np.exp(m_run - m_new)).astype(np.float32)
            if defect == "no_alpha" and k0 > 0:
                alpha = np.ones_like(alpha)
            l_run = l_run * alpha + l
            o = o * alpha[:, None] + _r(p, dtype) @ vb
            m_run = m_new
        out = np.where(l_run[:, None] > 0, o / l_run[:, None], np.float32(0))
        lse = (m_run + np.log(l_run)).astype(np.float32)
    return _r(out, dtype).astype(np.float64), lse.astype(np.float64)


def emu_bwd(q, k, v, out, dout, lse, allowed, dtype, *, block=None, defect=None):
    """single problem; block=None: the single-tile kernel; block=64: the two-pass walk (fp32 accumulators over the blocks).
    defect 'drop_last_q_block': dK / dV miss the last (ragged) 64-query block."""
    q, k, v, out, dout, lse = _f32(q, k, v, out, dout, lse)
    Tq, Tk = q.shape[0], k.shape[0]
    bq = block or Tq
    dq = np.zeros((Tq, D), np.float32)
    dk = np.zeros((Tk, D), np.float32)
    dv = np.zeros((Tk, D), np.float32)
    delta = (dout * out).sum(1, dtype=np.float32)
    nqb = (Tq + bq - 1) // bq
    with np.errstate(invalid="ignore", over="ignore"):
        for qi in range(nqb):
            r = slice(qi * bq, min(Tq, (qi + 1) * bq))
            s = (q[r] @ k.T) * np.float32(0.125)
            p = np.where(allowed[r], np.exp(s - lse[r, None]), np.float32(0)).astype(np.float32)
            ds = (p * ((dout[r] @ v.T) - delta[r, None]) * np.float32(0.125)).astype(np.float32)
            pt, dst = _r(p, dtype), _r(ds, dtype)
            dq[r] = dst @ k
            if defect == "drop_last_q_block" and qi == nqb - 1 and nqb > 1:
                continue
            dk += dst.T @ q[r]
            dv += pt.T @ dout[r]
    return tuple(_r(t, dtype).astype(np.float64) for t in (dq, dk, dv))


def emu_decode(q, kc, vc, H, max_len, cur, dtype, *, src_row=None, row_div=1, defect=None):
    """the decode kernels: 64-slot chunks with the running (max, sum, out) triple; p in registers (fp32).
    defect 'own_row_slot': slot 1 is read from cache row r instead of src_row[r][1]."""
    q, kc, vc = _f32(q, kc, vc)
    R = q.shape[0]
    n = min(cur + 1, max_len)
    out = np.zeros((R, H * D), np.float32)
    for r in range(R):
        rows = np.asarray(src_row[r][:n]).copy() if src_row is not None else np.full(n, r // row_div)
        if defect == "own_row_slot":
            rows[min(1, n - 1)] = r
        for h in range(H):
            c = slice(h * D, (h + 1) * D)
            qs = q[r, c] * np.float32(0.125)
            m_run, l_run, o = np.float32(-np.inf), np.float32(0), np.zeros(D, np.float32)
            for c0 in range(0, n, 64):
                sl = np.arange(c0, min(n, c0 + 64))
                s = kc[rows[sl], sl][:, c] @ qs
                m = np.maximum(m_run, s.max())
                p = np.exp(s - m).astype(np.float32)
                with np.errstate(invalid="ignore"):
                    alpha = np.exp(m_run - m).astype(np.float32)
                l_run = l_run * alpha + p.sum(dtype=np.float32)
                o = o * alpha + p @ vc[rows[sl], sl][:, c]
                m_run = m
            out[r, c] = o * (np.float32(1) / l_run)
    return _r(out, dtype).astype(np.float64)
