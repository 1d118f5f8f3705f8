"""fp64 references of the row operations on the training step's critical path — the LayerNorm family, the materialised-logits
cross-entropy family and AdamW — with a per-element error bound beside every quantity, and fp32 numpy emulations of the kernels'
arithmetic for the check on the checker (tests/test_rowop_conformance_{cpu,gpu}.py).  A helper module, not a conftest.

The references follow include/mic_hip.h, not the kernels, and work on the operands as stored (bf16 / fp32 values lifted to fp64).

Notation: u = storage roundoff (2^-8 bf16, 2^-24 fp32), u32 = 2^-24, gamma_n = 2 n u32 (util_gemm_ref.gamma_k: an fp32 sum of n
addends in ANY order), EPS_F = 32 u32 (__expf, logf, rsqrtf and the fp32 divisions).  W = width, R = rows.

LayerNorm forward (ln_fwd_ref)
    mean   e_mean = gamma_W sum|x| / W + u32 |mean|
    rstd   the kernel forms var^ = sum (x - mean^)^2 / W = var + (mean - mean^)^2 exactly, so e_mean enters in second order:
           e_var = e_mean^2 + (gamma_W + 4 u32) q,  q = sum (x - mean)^2 / W + e_mean^2  (one rounding of the difference, doubled by
           the square, one of the square, the sum, the division);  e_rstd = rstd (e_var / (2 (var + eps)) + u32 + EPS_F)
    y      e = |g| (rstd e_mean + |x - mean| e_rstd + 3 u32 |xhat|) + 2 u32 |y|;   stored: u |y| + (1 + u) e
    dropout (keep from mic_dropout_mask): kept v = y / (1 - p), e = e / (1 - p) + 2 u32 |v|, stored as above; dropped: exact 0

LayerNorm backward on the mean / rstd it is handed (ln_bwd_ref), d = dy (in_dropout: dy keep / (1 - p), + u32 |d|):
    h = (x - mean) rstd, gd = d g, c1 = sum gd / W, c2 = sum gd h / W
    e_c1 = (gamma_W + 3 u32) sum|gd| / W,  e_c2 = (gamma_W + 5 u32) sum|gd h| / W
    dx     e = rstd (e_c1 + |h| e_c2 + 4 u32 (|gd| + |c1| + |h c2|)) + u32 |o| (+ u32 |o + dres|);  stored: u |v| + (1 + u) e
    dxm    = stored dx * keep / (1 - p):  (u + 2 u32) |dxm|
    dgamma = sum_rows d h:  (gamma_R + 4 u32) sum|d h|;   dbeta = sum_rows d:  (gamma_R + u32) sum|d|
    end to end (statistics from the fp64 forward instead): the forward's e_mean, e_rstd move h by dh = rstd e_mean + |h| e_rstd / rstd,
    c2 by mean(|gd| dh), dx by |o| e_rstd / rstd + rstd (dh |c2| + |h| mean(|gd| dh));  dgamma by sum |d| dh.
    partials: the sum over blocks has the bound of dgamma / dbeta (same addends, another order).

mic_ln_fold_weight (fold_ref): w_fold = round(fl32(w gamma)) bit for bit (numpy's fp32 product is the kernel's);  colsum:
    gamma_K sum|w_fold|;  bias_fold: (gamma_K + 2 u32) (sum|w beta| + |bias|)

Cross-entropy (ce_rows_ref).  M = max x, p_i = exp(x_i - lse), n_r = rescales one addend passes through (ceil(chunks / 256) + 8 tree
levels; the arguments of one addend's exp and of its rescales add up to M - x_i):
    lse    e = sum_i p_i EPS_F (1 + n_r + M - x_i) + gamma_V + EPS_F (1 + |log s|) + u32 (|M| + |lse|)
    nll    = lse - x_label:  e_lse + u32 |nll|
    ls > 0 conf = 1 - ls, low = ls / (V - 1), norm = -(conf log conf + (V - 1) low log(low + 1e-20)), S = V lse - sum x:
           e_S = V e_lse + gamma_V sum|x| + 2 u32 (V |lse| + |S|)
           e = conf e_nll + low (e_S + e_nll) + 4 u32 (|conf nll| + |low (S - nll)| + |norm|) + EPS_F (|conf log conf| + |ls log low|)
               + u32 |loss|         (the cancellation in V lse - sum x at a large V is in e_S: V e_lse dominates)
    tiles  lse from (max, sum) partials as given: sum_g q_g EPS_F (1 + n_r + M - m_g) + gamma_ntiles + the log terms, n_r = trips + 1
    reduce denom exact;  loss: (gamma_R + 2 u32) sum|l mask| / denom + EPS_F |loss|
    dlogits = w (exp(x - lse) - soft) on the lse handed in, w = mask ? loss_scale / denom : 0:
           e = |w| (p EPS_F (1 + |x - lse|) + 2 u32 (p + soft)) + (EPS_F + u32) |v|;  stored: u |v| + (1 + u) e
           columns V .. Vpad exact zeros; a masked row all zero bits; an entry at -inf gives w (0 - low)
    colsum of mic_ce_bwd_t: start + sum of the STORED values: (gamma_R + u32) (sum|stored| + |start|)

AdamW (adamw_ref): fp64 of the header formula on the fp32 b1, b2, eps, wd, lr the kernel receives, (1 - b) = float32(1.0 - b):
    g' = g gscale;  e_m = 3 u32 (|b1 m| + |omb1 g'|);  e_v = 3 u32 b2 v + 5 u32 omb2 g'^2
    bc = 1 - b^t:  r_bc = (2 u32 b^t + u32) / (1 - b^t)   (large at t = 1 by construction: 1 - 0.999 keeps 14 bits)
    mhat: e_m / bc1 + (r_bc1 + EPS_F) |mhat|;  vhat likewise;  sqrt: e_vhat / (2 sqrt vhat) + 2 u32 sqrt vhat (vhat = 0: sqrt e_vhat)
    den = sqrt + eps: + u32 den;  q = mhat / den: e_mhat / den + |q| (e_den / den + EPS_F);  upd = q + wd p: + 2 u32 (|wd p| + |upd|)
    p' = p - lr upd:  lr e_upd + 2 u32 (|lr upd| + |p'|)

How tight (profiles/rowop_conformance_worst_ratio.txt; emulation and device agree to the second digit almost everywhere):
    - y, dx, dxm, dlogits in bf16 sit at 0.9 .. 0.995: the storage rounding is the bound; in fp32 they reach 0.03 .. 0.09.
    - AdamW's p / m / v 0.4 .. 0.6; dgamma / dbeta 0.3 .. 0.4 (at 3 rows, where gamma_R is not yet loose).
    - every bound led by a gamma_n term is loose by design: gamma_n = 2 n u32 holds for EVERY order of n addends, while the kernels add
      lane-strided partial sums and then a tree (error ~ (n / 64 + log 64) u32, and random signs on top).  That is mean (emulation
      worst 8e-4 bf16 / 9e-3 fp32 — below 0.01 everywhere: gamma_W over W = 8 .. 2048 against at most 32 + 6 sequential roundings),
      rstd (0.015), row_lse / row_loss (0.01 .. 0.02; at V = 250 054 gamma_V alone is 0.03 absolute, ratio 2e-5), colsum, bias_fold,
      loss.  They still reject what they are there for: a one-pass variance on a shifted row exceeds the rstd bound 15-fold and
      more, variance over W - 1, eps outside the root, a padded column in the CE row sum, low = ls / V, an omitted smoothing constant
      (tests/test_rowop_conformance_cpu.py).  A tighter, order-aware sum bound would have to restate each kernel's reduction tree, which
      is what the reference must not do.

Bound terms added after the first GPU run: none.
"""
from __future__ import annotations

import math

import numpy as np

from util_gemm_ref import EPS_F, U32, check, gamma_k, round_bf16, round_to, u_of  # noqa: F401

F = np.float32
NEG = -np.inf


def stored(t, dtype):
    """|stored - v| <= u |v| + (1 + u) e  as a function of (v, e)"""
    u = u_of(dtype)
    return lambda v, e: u * np.abs(v) + (1 + u) * e


def mic_hash(seed, idx):
    """common.h mic_hash on uint32 arrays"""
    with np.errstate(over="ignore"):
        s = np.uint32(seed)
        x = (idx.astype(np.uint32) * np.uint32(0x9E3779B1)) ^ s
        x ^= x >> np.uint32(16); x *= np.uint32(0x85EBCA6B); x ^= x >> np.uint32(13); x *= np.uint32(0xC2B2AE35); x ^= x >> np.uint32(16)  # noqa: E702
        x += s * np.uint32(0x27D4EB2F); x ^= x >> np.uint32(15); x *= np.uint32(0x2C1B3C6D); x ^= x >> np.uint32(12)  # noqa: E702
    return x


def keep_mask(n, p, seed):
    """the keep mask of mic_dropout_mask(seed, p) over n elements (bool)"""
    if p <= 0:
        return np.ones(n, bool)
    thr = np.uint32(min(float(F(p) * F(4294967296.0)), 4294967295.0))
    return mic_hash(seed, np.arange(n, dtype=np.uint32)) >= thr


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_fwd_ref(x, gamma, beta, eps, dtype, keep=None, p=0.0):
    x, g, b = (np.asarray(t, np.float64) for t in (x, gamma, beta))
    W = x.shape[1]
    gW = gamma_k(W)
    mean = x.mean(1)
    e_mean = gW * np.abs(x).sum(1) / W + U32 * np.abs(mean)
    d = x - mean[:, None]
    var = (d * d).mean(1)
    q = var + e_mean ** 2
    e_var = e_mean ** 2 + (gW + 4 * U32) * q
    rstd = 1.0 / np.sqrt(var + eps)
    e_rstd = rstd * (e_var / (2 * (var + eps)) + U32 + EPS_F)
    xh = d * rstd[:, None]
    y = xh * g + b
    e = np.abs(g) * (rstd[:, None] * e_mean[:, None] + np.abs(d) * e_rstd[:, None] + 3 * U32 * np.abs(xh)) + 2 * U32 * np.abs(y)
    if keep is not None and p > 0:
        sc = 1.0 / (1.0 - float(F(p)))
        k = np.asarray(keep, np.float64).reshape(x.shape)
        y = y * sc * k
        e = (e * sc + 2 * U32 * np.abs(y)) * k
    return dict(mean=mean, bound_mean=e_mean, rstd=rstd, bound_rstd=e_rstd, y=y, bound_y=stored(None, dtype)(y, e))


def ln_bwd_ref(x, gamma, mean, rstd, dy, dtype, dres=None, keep_in=None, p_in=0.0, fwd=None):
    """`fwd` (an ln_fwd_ref result whose mean / rstd were passed in): the end-to-end bound"""
    x, g, dy = (np.asarray(t, np.float64) for t in (x, gamma, dy))
    mu, rs = np.asarray(mean, np.float64)[:, None], np.asarray(rstd, np.float64)[:, None]
    R, W = x.shape
    gW, gR = gamma_k(W), gamma_k(R)
    d, e_d = dy, 0.0
    if keep_in is not None and p_in > 0:
        d = dy * np.asarray(keep_in, np.float64).reshape(x.shape) / (1.0 - float(F(p_in)))
        e_d = U32 * np.abs(d)
    h = (x - mu) * rs
    gd = d * g
    c1, c2 = gd.mean(1, keepdims=True), (gd * h).mean(1, keepdims=True)
    e_c1 = (gW + 3 * U32) * np.abs(gd).mean(1, keepdims=True)
    e_c2 = (gW + 5 * U32) * np.abs(gd * h).mean(1, keepdims=True)
    o = rs * (gd - c1 - h * c2)
    e = rs * (e_c1 + np.abs(h) * e_c2 + 4 * U32 * (np.abs(gd) + np.abs(c1) + np.abs(h * c2))) + U32 * np.abs(o)
    dg, db = (d * h).sum(0), d.sum(0)
    e_dg, e_db = (gR + 4 * U32) * np.abs(d * h).sum(0) + 1e-300, (gR + U32) * np.abs(d).sum(0) + 1e-300
    if fwd is not None:
        dh = rs * fwd["bound_mean"][:, None] + np.abs(h) * fwd["bound_rstd"][:, None] / rs
        e = e + np.abs(o) * fwd["bound_rstd"][:, None] / rs + rs * (dh * np.abs(c2) + np.abs(h) * (np.abs(gd) * dh).mean(1, keepdims=True))
        e_dg = e_dg + (np.abs(d) * dh).sum(0)
    if dres is not None:
        o = o + np.asarray(dres, np.float64)
        e = e + U32 * np.abs(o)
    return dict(dx=o, bound_dx=stored(None, dtype)(o, e + e_d * 0), dgamma=dg, bound_dgamma=e_dg, dbeta=db, bound_dbeta=e_db)


def dxm_ref(dx_stored, keep, p, dtype):
    v = np.asarray(dx_stored, np.float64) * np.asarray(keep, np.float64).reshape(np.shape(dx_stored)) / (1.0 - float(F(p)))
    return v, (u_of(dtype) + 2 * U32) * np.abs(v)


def fold_ref(w, gamma, beta, bias, dtype):
    """(w_fold exact, colsum, bound, bias_fold, bound)"""
    w32, K = np.asarray(w, F), np.shape(w)[1]
    wf = round_to((w32 * np.asarray(gamma, F)[None, :]).astype(np.float64), dtype)
    w64, be = w32.astype(np.float64), np.asarray(beta, np.float64)
    bz = np.zeros(w32.shape[0]) if bias is None else np.asarray(bias, np.float64)
    bf = bz + (w64 * be).sum(1)
    return (wf, wf.sum(1), gamma_k(K) * np.abs(wf).sum(1) + 1e-300, bf,
            (gamma_k(K) + 2 * U32) * (np.abs(w64 * be).sum(1) + np.abs(bz)) + 1e-300)


# ------------------------------------------------------------------------------------------------ cross-entropy
def _lse(x):
    M = x.max(1)
    with np.errstate(invalid="ignore"):
        s = np.exp(x - M[:, None]).sum(1)
    return M, s, M + np.log(s)


def ce_rows_ref(x, labels, ls):
    """x fp64 [rows][V] (stored values; -inf allowed, every row has a finite entry) -> lse, row_loss and their bounds"""
    x = np.asarray(x, np.float64)
    R, V = x.shape
    M, s, lse = _lse(x)
    n_r = -(-((V + 7) // 8) // 256) + 8
    p = np.exp(x - lse[:, None])
    gap = np.where(p > 0, M[:, None] - x, 0.0)
    e_lse = (p * EPS_F * (1 + n_r + gap)).sum(1) + gamma_k(V) + EPS_F * (1 + np.abs(np.log(s))) + U32 * (np.abs(M) + np.abs(lse))
    xl = x[np.arange(R), labels]
    nll = lse - xl
    e_nll = e_lse + U32 * np.abs(nll)
    if not ls > 0:
        return dict(lse=lse, bound_lse=e_lse, loss=nll, bound_loss=e_nll)
    ls = float(F(ls))
    conf, low = 1.0 - ls, ls / (V - 1)
    norm = -(conf * math.log(conf) + (V - 1) * low * math.log(low + 1e-20))
    S = V * lse - x.sum(1)
    e_S = V * e_lse + gamma_k(V) * np.abs(x).sum(1) + 2 * U32 * (V * np.abs(lse) + np.abs(S))
    loss = conf * nll + low * (S - nll) - norm
    e = (conf * e_nll + low * (e_S + e_nll) + 4 * U32 * (np.abs(conf * nll) + np.abs(low * (S - nll)) + abs(norm))
         + EPS_F * (abs(conf * math.log(conf)) + abs(ls * math.log(low))) + U32 * np.abs(loss))
    return dict(lse=lse, bound_lse=e_lse, loss=loss, bound_loss=e)


def tile_partials(x):
    """(max, sum exp(x - max)) per 64-column granule of x [rows][V], rounded to fp32: [rows][ntiles][2]; a granule of -inf gives (-inf, 0)"""
    x = np.asarray(x, np.float64)
    R, V = x.shape
    nt = (V + 63) // 64
    xp = np.full((R, nt * 64), NEG)
    xp[:, :V] = x
    G = xp.reshape(R, nt, 64)
    m = G.max(2)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isfinite(m), np.exp(G - np.where(np.isfinite(m), m, 0.0)[..., None]).sum(2), 0.0)
    return np.stack([m, s], 2).astype(F)


def ce_tiles_ref(part, x_label):
    """lse / nll from the fp32 partials as given"""
    m, s = part[..., 0].astype(np.float64), part[..., 1].astype(np.float64)
    nt = m.shape[1]
    M = m.max(1)
    with np.errstate(invalid="ignore"):
        q = np.where(s > 0, s * np.exp(m - M[:, None]), 0.0)
    tot = q.sum(1)
    lse = M + np.log(tot)
    n_r = -(-nt // 256) + 1
    gap = np.where(q > 0, M[:, None] - m, 0.0)
    e = ((q / tot[:, None]) * EPS_F * (1 + n_r + gap)).sum(1) + gamma_k(nt) + EPS_F * (1 + np.abs(np.log(tot))) + U32 * (np.abs(M) + np.abs(lse))
    nll = lse - np.asarray(x_label, np.float64)
    return dict(lse=lse, bound_lse=e, loss=nll, bound_loss=e + U32 * np.abs(nll))


def ce_reduce_ref(row_loss, mask):
    l, m = np.asarray(row_loss, np.float64), np.asarray(mask, np.float64)
    den = m.sum()
    loss = (l * m).sum() / den
    return loss, (gamma_k(len(l)) + 2 * U32) * np.abs(l * m).sum() / den + EPS_F * abs(loss) + 1e-300, den


def ce_bwd_ref(x, V, labels, mask, ls, lse, denom, loss_scale, dtype):
    """x fp64 [rows][Vpad] as stored (columns >= V: anything) -> dlogits [rows][Vpad] and its bound"""
    x = np.asarray(x, np.float64)
    R, Vp = x.shape
    lsf = float(F(ls))
    conf, low = 1.0 - lsf, (lsf / (V - 1) if ls > 0 else 0.0)
    w = np.where(np.asarray(mask) != 0, float(F(loss_scale)) / float(denom), 0.0)[:, None]
    soft = np.full((R, V), low)
    soft[np.arange(R), labels] = conf
    a = x[:, :V] - np.asarray(lse, np.float64)[:, None]
    p = np.exp(a)
    v = np.zeros((R, Vp))
    e = np.zeros((R, Vp))
    v[:, :V] = w * (p - soft)
    e[:, :V] = np.abs(w) * (p * EPS_F * (1 + np.where(p > 0, np.abs(a), 0.0)) + 2 * U32 * (p + soft)) + (EPS_F + U32) * np.abs(v[:, :V])
    return v, stored(None, dtype)(v, e)


CANARY16 = 0x7FA5


def emu_transpose(src_bits, rows_pad, ld_t, defect=None):
    """tile_transpose_kernel on uint16 bits: dst [cols][ld_t] in a canary-filled allocation.  defect: 'no_pad'"""
    rows, cols = src_bits.shape
    t = np.full((cols, ld_t), CANARY16, np.uint16)
    t[:, :rows] = src_bits.T
    if defect != "no_pad":
        t[:, rows:rows_pad] = 0
    return t


def check_transposed(t_bits, src_bits, rows, rows_pad):
    """t [cols][ld_t] is bit for bit the transpose of src [rows][cols]; columns rows .. rows_pad zero bits; the rest canary"""
    assert np.array_equal(t_bits[:, :rows], src_bits.T), "dlogits_t is not the transpose of the stored dlogits"
    assert not t_bits[:, rows:rows_pad].any(), "columns rows .. rows_pad of the transposed copy are not zero"
    assert (t_bits[:, rows_pad:] == CANARY16).all(), "columns rows_pad .. ld_t of the transposed copy were written"


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_consts(b1, b2, eps, wd):
    """what the entry point hands the kernel: (b1, b2, 1 - b1, 1 - b2, eps, wd) as fp32 values, the differences formed in double"""
    return tuple(float(F(t)) for t in (b1, b2, 1.0 - b1, 1.0 - b2, eps, wd))


def adamw_ref(p, m, v, g, lr, t, b1, b2, eps, wd, gscale=1.0):
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    b1, b2, o1, o2, eps, wd = adamw_consts(b1, b2, eps, wd)
    lr, t, gs = float(F(lr)), float(F(t)), float(F(gscale))
    gp = g * gs
    m2 = b1 * m + o1 * gp
    e_m = 3 * U32 * (np.abs(b1 * m) + np.abs(o1 * gp))
    v2 = b2 * v + o2 * gp * gp
    e_v = 3 * U32 * b2 * v + 5 * U32 * o2 * gp * gp
    p1, p2 = b1 ** t, b2 ** t
    bc1, bc2 = 1 - p1, 1 - p2
    r1, r2 = (2 * U32 * p1 + U32) / bc1, (2 * U32 * p2 + U32) / bc2
    mh, vh = m2 / bc1, v2 / bc2
    e_mh, e_vh = e_m / bc1 + (r1 + EPS_F) * np.abs(mh), e_v / bc2 + (r2 + EPS_F) * vh
    sq = np.sqrt(vh)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_sq = np.where(vh > 0, e_vh / (2 * np.where(sq > 0, sq, 1.0)), np.sqrt(e_vh)) + 2 * U32 * sq
    den = sq + eps
    e_den = e_sq + U32 * den
    q = mh / den
    e_q = e_mh / den + np.abs(q) * (e_den / den + EPS_F)
    upd = q + wd * p
    e_u = e_q + 2 * U32 * (np.abs(wd * p) + np.abs(upd))
    pn = p - lr * upd
    e_p = lr * e_u + 2 * U32 * (np.abs(lr * upd) + np.abs(pn))
    z = 1e-300
    return dict(p=pn, bound_p=e_p + z, m=m2, bound_m=e_m + z, v=v2, bound_v=e_v + z)


# ------------------------------------------------------------------------------------------------ fp32 emulations of the kernels
def rnd(x, dtype):
    """fp32 array -> the stored value (fp32 array)"""
    return round_bf16(x.astype(np.float64)).astype(F) if dtype == "bf16" else x.astype(F)


def _xor_tree(a):
    """wave_sum: a [..., 64] fp32 -> [...] by xor-shuffle halving"""
    a = a.astype(F)
    o = 32
    while o:
        a = (a.reshape(a.shape[:-1] + (-1, 2, o))[..., 0, :] + a.reshape(a.shape[:-1] + (-1, 2, o))[..., 1, :]).reshape(a.shape[:-1] + (-1,))
        o >>= 1
    return a[..., 0]


def _lanes(x):
    """[R][W] -> [R][64][nc*8] fp32: lane l holds chunks l, l + 64, ... (absent chunks 0) in the kernel's visiting order"""
    R, W = x.shape
    nc = -(-(W // 8) // 64)
    xp = np.zeros((R, nc * 512), F)
    xp[:, :W] = x
    return xp.reshape(R, nc, 64, 8).transpose(0, 2, 1, 3).reshape(R, 64, nc * 8)


def _seqsum(a):
    """sequential fp32 sum over the last axis"""
    s = np.zeros(a.shape[:-1], F)
    for i in range(a.shape[-1]):
        s = (s + a[..., i]).astype(F)
    return s


def emu_ln_fwd(x, gamma, beta, eps, dtype, keep=None, p=0.0, defect=None):
    """ln_fwd_kernel: lane-strided partial sums, xor tree, two-pass variance.  defect: 'one_pass' | 'w_minus_1' | 'eps_outside' | 'no_scale'"""
    x = np.asarray(x, F)
    R, W = x.shape
    g, b = np.asarray(gamma, F), np.asarray(beta, F)
    L = _lanes(x)
    valid = _lanes(np.ones((1, W), F))[0] > 0
    mean = (_xor_tree(_seqsum(L)) / F(W)).astype(F)
    if defect == "one_pass":
        var = ((_xor_tree(_seqsum((L * L).astype(F))) / F(W)).astype(F) - (mean * mean).astype(F)).astype(F)
    else:
        d = np.where(valid, (L - mean[:, None, None]).astype(F), F(0))
        var = (_xor_tree(_seqsum((d * d).astype(F))) / F(W - 1 if defect == "w_minus_1" else W)).astype(F)
    if defect == "eps_outside":
        rstd = (F(1) / (np.sqrt(var).astype(F) + F(eps))).astype(F)
    else:
        rstd = (F(1) / np.sqrt((var + F(eps)).astype(F), dtype=F)).astype(F)
    y = ((((x - mean[:, None]).astype(F) * rstd[:, None]).astype(F) * g).astype(F) + b).astype(F)
    if keep is not None and p > 0:
        sc = F(1) if defect == "no_scale" else (F(1) / (F(1) - F(p))).astype(F)
        y = np.where(np.asarray(keep).reshape(x.shape), (y * sc).astype(F), F(0))
    return rnd(y, dtype), mean, rstd


def emu_ln_bwd(x, gamma, mean, rstd, dy, dtype, dres=None, keep_in=None, p_in=0.0, nblk=None, defect=None):
    """ln_bwd_kernel: dx rows as the kernel forms them; dgamma / dbeta per wave over its rows (row = (blk * 8 + wave) + k * nblk * 8),
    the block's 8 waves in order, the blocks in order.  defect: 'no_dres' | 'no_c2_last' | 'no_carry'"""
    x, dy, g = np.asarray(x, F), np.asarray(dy, F), np.asarray(gamma, F)
    R, W = x.shape
    mu, rs = np.asarray(mean, F)[:, None], np.asarray(rstd, F)[:, None]
    d = dy
    if keep_in is not None and p_in > 0:
        d = np.where(np.asarray(keep_in).reshape(x.shape), (dy * (F(1) / (F(1) - F(p_in)))).astype(F), F(0))
    h = ((x - mu).astype(F) * rs).astype(F)
    gd = (d * g).astype(F)
    c1 = (_xor_tree(_seqsum(_lanes(gd))) / F(W)).astype(F)[:, None]
    c2 = (_xor_tree(_seqsum(_lanes((gd * h).astype(F)))) / F(W)).astype(F)[:, None]
    hc = (h * c2).astype(F)
    if defect == "no_c2_last":
        last = ((np.arange(W) // 8) // 64) == ((W // 8 - 1) // 64)
        hc = np.where(last[None, :], F(0), hc)
    o = (rs * ((gd - c1).astype(F) - hc).astype(F)).astype(F)
    if dres is not None and defect != "no_dres":
        o = (o + np.asarray(dres, F)).astype(F)
    nblk = nblk or min(-(-R // 8), 512)
    slots = nblk * 8
    trips = -(-R // slots)
    dh = (d * h).astype(F)
    accg, accb = np.zeros((slots, W), F), np.zeros((slots, W), F)
    for k in range(trips):
        rows = np.arange(k * slots, min((k + 1) * slots, R))
        if defect == "no_carry" and k:
            accg[:len(rows)] = 0
        accg[:len(rows)] = (accg[:len(rows)] + dh[rows]).astype(F)
        accb[:len(rows)] = (accb[:len(rows)] + d[rows]).astype(F)
    part = np.stack([_seqsum(a.reshape(nblk, 8, W).transpose(0, 2, 1)) for a in (accg, accb)])  # [2][nblk][W]
    return rnd(o, dtype), _seqsum(part[0].T), _seqsum(part[1].T), part


def _expf(x):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(np.asarray(x, F), dtype=F)


def _merge(m, s, m2, s2):
    mn = np.maximum(m, m2)
    dead = np.isneginf(mn)
    safe = np.where(dead, F(0), mn)
    out = ((s * _expf(np.where(dead, F(0), m - safe))).astype(F) + (s2 * _expf(np.where(dead, F(0), m2 - safe))).astype(F)).astype(F)
    return mn, np.where(dead, F(0), out)


def emu_ce_rows(x, labels, ls, defect=None, guard=True):
    """ce_rows_kernel: per-thread online (max, sum exp, sum) over chunks tid, tid + 256, ..., then the LDS halving tree.
    guard=False: the loop as it was before this suite (exp(-inf - -inf) on a chunk of -inf).  defect: 'pad_in_sum' (x needs one more
    column) | 'low_over_v' | 'no_norm'"""
    x = np.asarray(x, F)
    R, V = x.shape[0], x.shape[1] - (1 if defect == "pad_in_sum" else 0)
    nch = (V + 7) // 8
    trips = -(-nch // 256)
    xp = np.full((R, trips * 2048), F(NEG))
    xp[:, :V] = x[:, :V]
    tp = np.zeros((R, trips * 2048), F)
    tp[:, :x.shape[1]] = np.where(np.isfinite(x), x, x)
    if defect != "pad_in_sum":
        tp[:, V:] = 0
    C = xp.reshape(R, trips, 256, 8)
    T = tp.reshape(R, trips, 256, 8)
    m, s, tot = np.full((R, 256), F(NEG)), np.zeros((R, 256), F), np.zeros((R, 256), F)
    for k in range(trips):
        present = (np.arange(256) + k * 256 < nch)[None, :]
        cm = C[:, k].max(2)
        mn = np.maximum(m, cm)
        with np.errstate(invalid="ignore"):
            if guard:
                dead = np.isneginf(mn)
                base = np.where(dead, F(0), mn)
                add = _seqsum(np.where(np.isneginf(C[:, k]), F(0), _expf(C[:, k] - base[..., None])))
                s2 = np.where(dead, F(0), ((s * _expf(np.where(dead, F(0), m - base))).astype(F) + add).astype(F))
            else:
                add = _seqsum(np.where((np.arange(k * 2048, (k + 1) * 2048) < V).reshape(1, 256, 8), _expf(C[:, k] - mn[..., None]), F(0)))
                s2 = ((s * _expf(m - mn)).astype(F) + add).astype(F)
        s = np.where(present, s2, s)
        m = np.where(present, mn, m)
        for i in range(8):
            tot = (tot + T[:, k, :, i]).astype(F)
    o = 128
    while o:
        mm, ss = _merge(m[:, :o], s[:, :o], m[:, o:2 * o], s[:, o:2 * o])
        tot = (tot[:, :o] + tot[:, o:2 * o]).astype(F)
        m, s = mm, ss
        o >>= 1
    lse = (m[:, 0] + np.log(s[:, 0], dtype=F)).astype(F)
    nll = (lse - x[np.arange(R), labels]).astype(F)
    if not ls > 0:
        return lse, nll
    ls = F(ls)
    conf, low = F(1) - ls, (ls / F(V if defect == "low_over_v" else V - 1)).astype(F)
    norm = F(0) if defect == "no_norm" else -(conf * np.log(conf, dtype=F) + F(V - 1) * low * np.log(low + F(1e-20), dtype=F)).astype(F)
    S = ((F(V) * lse).astype(F) - tot[:, 0]).astype(F)
    return lse, (((conf * nll).astype(F) + (low * (S - nll).astype(F)).astype(F)).astype(F) - norm).astype(F)


def emu_ce_tiles(part, x_label, aligned):
    """ce_rows_tiles_kernel: the 4-pair trip (aligned) or one pair per trip, then the wave's max and sum"""
    R, nt = part.shape[:2]
    step = 256 if aligned else 64
    trips = -(-nt // step)
    P = np.zeros((R, trips * step, 2), F)
    P[..., 0] = NEG
    P[:, :nt] = part
    m, s = np.full((R, 64), F(NEG)), np.zeros((R, 64), F)
    for k in range(trips):
        if aligned:
            blk = P[:, k * 256:(k + 1) * 256].reshape(R, 64, 4, 2)
            mn = np.maximum(m, blk[..., 0].max(2))
            dead = np.isneginf(mn)
            base = np.where(dead, F(0), mn)[..., None]
            t = np.where(np.isneginf(blk[..., 0]), F(0), (blk[..., 1] * _expf(np.where(np.isneginf(blk[..., 0]), F(0), blk[..., 0] - base))).astype(F))
            add = ((t[..., 0] + t[..., 1]).astype(F) + (t[..., 2] + t[..., 3]).astype(F)).astype(F)
            s = np.where(dead, s, ((s * _expf(np.where(np.isneginf(m), F(NEG), m - base[..., 0]))).astype(F) + add).astype(F))
            m = mn
        else:
            blk = P[:, k * 64:(k + 1) * 64]
            m, s = _merge(m, s, blk[..., 0], blk[..., 1])
    M = m.max(1)
    s = _xor_tree(np.where(np.isneginf(m), F(0), (s * _expf(np.where(np.isneginf(m), F(0), m - M[:, None]))).astype(F)))
    lse = (M + np.log(s, dtype=F)).astype(F)
    return lse, (lse - np.asarray(x_label, F)).astype(F)


def emu_ce_bwd(x, V, labels, mask, ls, lse, denom, loss_scale, dtype, defect=None):
    """ce_bwd_kernel on stored x [rows][Vpad].  defect: 'label_late' (label matched one column late at a chunk edge) | 'masked_grad'"""
    x = np.asarray(x, F)
    R, Vp = x.shape
    ls = F(ls)
    conf, low = F(1) - ls, ((ls / F(V - 1)).astype(F) if ls > 0 else F(0))
    mk = np.asarray(mask) != 0
    if defect == "masked_grad":
        mk = np.ones_like(mk)
    w = np.where(mk, (F(loss_scale) / F(denom)).astype(F), F(0))[:, None]
    lab = np.asarray(labels).copy()
    if defect == "label_late":
        lab = np.where(lab % 8 == 7, lab + 1, lab)
    soft = np.full((R, Vp), low, F)
    ok = lab < Vp
    soft[np.arange(R)[ok], lab[ok]] = conf
    with np.errstate(invalid="ignore"):
        o = (w * (_expf(x - np.asarray(lse, F)[:, None]) - soft).astype(F)).astype(F)
    o[:, V:] = 0
    return rnd(np.where(mk[:, None], o, F(0)), dtype)


def emu_adamw(p, m, v, g, lr, t, b1, b2, eps, wd, gscale=1.0, defect=None):
    """adamw_kernel's operation order.  defect: 't_minus_1' | 'eps_inside' | 'coupled_wd' | 'omb2_f32'"""
    p, m, v, g = (np.asarray(a, F) for a in (p, m, v, g))
    b1f, b2f, o1, o2, epsf, wdf = (F(c) for c in adamw_consts(b1, b2, eps, wd))
    if defect == "omb2_f32":
        o2 = F(1) - b2f
    tt = F(t) - (F(1) if defect == "t_minus_1" else F(0))
    bc1 = F(1) - F(float(b1f) ** float(tt))
    bc2 = F(1) - F(float(b2f) ** float(tt))
    ga = (g * F(gscale)).astype(F)
    if defect == "coupled_wd":
        ga = (ga + wdf * p).astype(F)
    m2 = ((b1f * m).astype(F) + (o1 * ga).astype(F)).astype(F)
    v2 = ((b2f * v).astype(F) + ((o2 * ga).astype(F) * ga).astype(F)).astype(F)
    vh = (v2 / bc2).astype(F)
    den = np.sqrt((vh + epsf * epsf).astype(F), dtype=F) if defect == "eps_inside" else (np.sqrt(vh, dtype=F) + epsf).astype(F)
    upd = ((m2 / bc1).astype(F) / den).astype(F)
    if defect != "coupled_wd":
        upd = (upd + (wdf * p).astype(F)).astype(F)
    return (p - (F(lr) * upd).astype(F)).astype(F), m2, v2
