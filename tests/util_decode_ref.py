"""fp64 references of the selection kernels of csrc/decode.hip — mic_row_lse_topk, mic_row_forced_topk, mic_row_topk_tiles,
mic_warp_thresholds, mic_sample_rows, mic_greedy_step — with a derived bound beside every value, the admissibility tests that say
where an fp64 order is the truth for an fp32 kernel, and fp32 numpy emulations of the kernels' arithmetic for the check on the
checker (tests/test_decode_conformance_{cpu,gpu}.py).  A helper module, not a conftest.

The references follow include/mic_hip.h and the Flax processors / warpers (oracle/generation_ref.py), not the kernels, and work on
the logits as stored (bf16 / fp32 values lifted to fp64).  Notation as in util_rowop_ref: u32 = 2^-24, gamma_n = 2 n u32 (an fp32
sum of n addends in any order), EPS_F = 32 u32 (__expf, logf).

Processed value of mic_row_lse_topk / mic_row_topk_tiles (proc_ref): lp = x - lse, + bias; EOS := -inf when suppressed.
    M = max x, s = sum exp(x - M), p_i = exp(x_i - M) / s, n_r = rescales one addend passes through (streaming kernel: passes of
    8192 columns + 8 tree levels; tiles: 1).  The kernel keeps M (exact) and log s apart and forms ((x - M) - log s) + bias:
    e_ls  = sum_i p_i EPS_F (1 + n_r + M - x_i) + gamma_V + EPS_F (1 + |log s|)         (tiles: gamma_ntiles + u32, the partial sums
            as stored in fp32, and M - m_g of the granule in place of M - x_i)
    b     = e_ls + u32 (|x - M| + |lp|) (+ u32 |lp + bias| when there is a bias)
    raw_logits: fp32(x + bias), one rounding of an exact sum, compared bit for bit (b = 0).  With k = 1 mic_row_lse_topk is the
    greedy argmax: the first maximum of the logits themselves, its value + bias (mic_row_topk_tiles orders by x + bias at every k; the
    two differ only where a bias merges distinct logits).
    |bias| >= 1e6 (NEG_BIG: ulp 1): the kernel's value is fp32(lp32 + bias); where lp + bias is further than b from an fp32 rounding
    boundary that is fp32(lp + bias) exactly — the key of the order and the value compared bit for bit.

Order (admissible_topk).  The kernels order by their own fp32 value, ties to the lower index.  Contenders = elements whose fp64 value
is >= the k-th best - b.  Rule 1: two contenders with different input logits differ by more than 2 b (equal logits are exact ties in
any monotone arithmetic).  Rule 2 (rows of a large bias): no finite element of the row within b of a rounding boundary.

Top-p (warp_ref): position j of the descending order is kept iff j == 0 or mass_before(j) / Z < top_p.  The kernel compares
fixed-point masses floor(expf(v - mx) 2^40), summed exactly: each mass is off by e_i EPS_F (1 + |v_i - mx|) + 2^-40, so mass_before / Z
moves by at most delta = 2 (sum_i e_i EPS_F (1 + |v_i - mx|) + (V + 1) 2^-40) / Z  (numerator and denominator, the ceiling of the
target).  Admissible: no position within delta of top_p.

Sampling (sample_ref): y = fp32(x / T) is a correctly rounded division and exact in numpy; u comes from the bits exactly;
g = -log(-log u) through two logf.  logf is accurate in the relative sense over its whole domain (also next to 1, where l = -log u
is small — and g large, the likely winner — an absolute bound would be useless), so |l32 - l| <= EPS_F l and
|g32 - g| <= EPS_F (1 + |log l|) = EPS_F (1 + |g|);  b_i = EPS_F (1 + |g_i|) + u32 |y_i + g_i|.  Admissible: best - second > b_best +
b_second.

Bound terms added after the first GPU run: none.
"""
from __future__ import annotations

import math

import numpy as np

from util_gemm_ref import EPS_F, U32, check, gamma_k, round_to  # noqa: F401

F = np.float32
NEG = -np.inf
NOIDX = 0x7FFFFFFF
BIG_BIAS = 1e6


def order(keys, k, highest_index=False):
    """the first k of (value desc, index asc) — lax.top_k"""
    keys = np.asarray(keys, np.float64)
    idx = np.arange(keys.size)
    o = np.lexsort((-idx if highest_index else idx, -keys))
    return o[:k]


# ------------------------------------------------------------------------------------------------ log-softmax + top-k
def lse_ref(x, n_r):
    """(lse, M, log s, e_ls) of one row; -inf entries carry no mass"""
    x = np.asarray(x, np.float64)
    M = x.max()
    with np.errstate(invalid="ignore"):
        e = np.where(np.isfinite(x), np.exp(x - M), 0.0)
        d = np.where(np.isfinite(x), M - x, 0.0)
    s = e.sum()
    p = e / s
    e_ls = float((p * EPS_F * (1 + n_r + d)).sum() + gamma_k(x.size) + EPS_F * (1 + abs(math.log(s))))
    return M + math.log(s), M, math.log(s), e_ls


def lse_tiles_ref(part):
    """the same from the (max, sum) partials of one row as given ([ntiles][2], the sums as stored in fp32)"""
    m, q = np.asarray(part[:, 0], np.float64), np.asarray(part[:, 1], np.float64)
    M = m.max()
    with np.errstate(invalid="ignore"):
        w = np.where(np.isfinite(m), q * np.exp(m - M), 0.0)
        d = np.where(np.isfinite(m), M - m, 0.0)
    s = w.sum()
    e_ls = float((w / s * EPS_F * (2 + d)).sum() + gamma_k(m.size) + U32 + EPS_F * (1 + abs(math.log(s))))
    return M + math.log(s), M, math.log(s), e_ls


def streaming_rescales(V):
    return -(-((V + 7) // 8) // 1024) + 8


def proc_ref(x, bias=0.0, *, suppress_eos=False, eos=2, raw=False, part=None):
    """one row: dict(v = fp64 processed values, b = bound on the kernel's fp32 value, key = what the order is taken on, exact = the
    value is compared bit for bit, x = the logits with the EOS column at -inf (what rule 1 compares))"""
    x = np.asarray(x, np.float64).copy()
    bias = float(F(bias))
    xe = x.copy()
    if suppress_eos and 0 <= eos < x.size:
        xe[eos] = NEG
    if raw:
        with np.errstate(invalid="ignore"):
            v = (xe.astype(F) + F(bias)).astype(np.float64)
        return dict(v=v, b=np.zeros_like(v), key=v, exact=True, x=xe, argmax_key=None if part is not None else xe)
    lse, M, ls, e_ls = lse_tiles_ref(part) if part is not None else lse_ref(x, streaming_rescales(x.size))
    fin = np.isfinite(xe)
    lp = np.where(fin, xe - lse, NEG)
    v = np.where(fin, lp + bias, NEG)
    with np.errstate(invalid="ignore"):
        b = np.where(fin, e_ls + U32 * (np.abs(xe - M) + np.abs(lp)), 0.0)
    if abs(bias) >= BIG_BIAS:  # b bounds lp32; the last rounding is part of the key
        return dict(v=v, b=b, key=v.astype(F).astype(np.float64), exact=True, x=xe)
    if bias != 0:
        b = b + np.where(fin, U32 * np.abs(np.where(fin, v, 0.0)), 0.0)
    return dict(v=v, b=b, key=v, exact=False, x=xe)


def boundary_distance(v):
    """distance of fp64 values to the nearest fp32 rounding boundary"""
    f = np.asarray(v, np.float64).astype(F)
    up, dn = np.nextafter(f, F(np.inf)).astype(np.float64), np.nextafter(f, F(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    return np.minimum(np.abs((f + up) / 2 - v), np.abs((f + dn) / 2 - v))


def admissible_topk(r, k, raw=False):
    """violations of rules 1 and 2 on one row of proc_ref (an empty list: the fp64 order is the truth)"""
    v, b, fin = r["v"], r["b"], np.isfinite(r["v"])
    if raw or not fin.any():
        return []
    if r["exact"]:  # rule 2
        d = boundary_distance(v[fin])
        bad = d <= b[fin]
        return [f"{int(bad.sum())} elements within b of an fp32 rounding boundary (closest {d.min():.3g}, b {b[fin].max():.3g})"] if bad.any() else []
    kth = np.sort(v)[::-1][min(k, v.size) - 1]
    bmax = b[fin].max()
    cont = fin & (v >= kth - bmax) if np.isfinite(kth) else fin
    ux = np.unique(r["x"][cont])
    if ux.size > 1 and not np.diff(ux).min() > 2 * bmax:
        return [f"two contenders with different logits {np.diff(ux).min():.3g} apart, 2 b = {2 * bmax:.3g}"]
    return []


def topk_ref(r, k):
    """(values, indices, bounds) of the first k in the reference order"""
    first_max = k == 1 and r.get("argmax_key") is not None  # mic_row_lse_topk, raw_logits, k = 1: argmax of the logits, + bias
    i = order(r["argmax_key"] if first_max else r["key"], k)
    return r["key"][i], i, r["b"][i]


def forced_ref(V, forced, k, bias=0.0):
    """ForcedBOS / ForcedEOS (everything -inf, the forced token 0) + bias, then top-k"""
    s = np.full(V, NEG)
    s[forced] = 0.0
    with np.errstate(invalid="ignore"):
        s = (s.astype(F) + F(bias)).astype(np.float64)
    i = order(s, k)
    return s[i], i


def check_topk(got_val, got_idx, r, k, V, what, quantity, log=True):
    """the demands on an admissible row: the reference's index sequence, isfinite patterns, indices distinct and < V, values within b
    (bit for bit where the reference is exact).  Returns the worst err / bound (None: compared exactly)."""
    rv, ri, rb = topk_ref(r, k)
    got_val, got_idx = np.asarray(got_val, np.float64), np.asarray(got_idx, np.int64)
    assert got_idx.size == k and np.unique(got_idx).size == k and (got_idx >= 0).all() and (got_idx < V).all(), f"{what}: indices {got_idx.tolist()}"
    assert np.array_equal(got_idx, ri), f"{what}: indices {got_idx.tolist()} reference {ri.tolist()}"
    assert np.array_equal(np.isfinite(got_val), np.isfinite(rv)) and not np.isnan(got_val).any(), f"{what}: isfinite pattern"
    f = np.isfinite(rv)
    assert (got_val[~f] == NEG).all(), f"{what}: a value that is not -inf where the reference is"
    if r["exact"]:
        assert np.array_equal(got_val[f], rv[f]), f"{what}: values {got_val[f].tolist()} reference {rv[f].tolist()}"
        return None
    return check(got_val[f], rv[f], rb[f], f"{quantity}: {what}", log=log) if f.any() else 0.0


# ------------------------------------------------------------------------------------------------ warpers
def scaled(x, temperature, suppress_eos=False, eos=2):
    """fp32(x / T) (a correctly rounded division: the kernel's bits), EOS := -inf, as float64"""
    y = np.asarray(x, np.float64).astype(F)
    if F(temperature) != F(1.0):
        y = (y / F(temperature)).astype(F)
    y = y.astype(np.float64) + 0.0
    y[y == 0] = 0.0
    if suppress_eos and 0 <= eos < y.size:
        y[eos] = NEG
    return y


def warp_ref(y, top_k, top_p):
    """one row of scaled scores -> dict(keep = the fp64 warpers' mask, n_topk = entries top-k leaves, margin / delta = distance of the
    closest sorted position's mass_before / Z to top_p and the derived delta (None without top-p))"""
    y = np.asarray(y, np.float64)
    V = y.size
    keep = np.isfinite(y)
    if top_k and top_k > 0:
        sel = np.zeros(V, bool)
        sel[order(y, min(int(top_k), V))] = True
        keep &= sel
    n_topk = int(keep.sum())
    margin = delta = None
    p = float(F(top_p))
    if p < 1.0:
        o = order(np.where(keep, y, NEG), n_topk)
        v = y[o]
        e = np.exp(v - v[0])
        Z = e.sum()
        before = (np.cumsum(e) - e) / Z
        kept = before < p
        kept[0] = True
        delta = 2 * ((e * EPS_F * (1 + np.abs(v - v[0]))).sum() + (V + 1) * 2.0 ** -40) / Z
        margin = float(np.abs(before[1:] - p).min()) if v.size > 1 else np.inf
        keep = np.zeros(V, bool)
        keep[o[kept]] = True
    return dict(keep=keep, n_topk=n_topk, margin=margin, delta=delta)


def mask_of(y, thr, lim):
    """the keep mask a (thr, tie_limit) pair stands for, over the finite entries"""
    y = np.asarray(y, np.float64)
    return np.isfinite(y) & ((y > thr) | ((y == thr) & (np.arange(y.size) < lim)))


# ------------------------------------------------------------------------------------------------ sampling
def kernel_bits(key, n, defect=None):
    """the threefry word of element e as the kernel picks it (counter array padded to even, split in halves x0 | x1)"""
    from oracle import generation_ref as G

    e = np.arange(n, dtype=np.uint64)
    h = (n + 1) // 2 if defect != "halves_swapped" else n // 2  # the defect: the split at floor(n / 2), so at an odd n the pad
    lo = e < h                                                  # counter sits in the other half; an even n is not affected
    c0 = np.where(lo, e, e - h)
    c1 = np.where(lo, np.where(e + h < n, e + h, 0), e)
    a, b = G.threefry2x32(key, c0.astype(np.uint32), c1.astype(np.uint32))
    return np.where(lo, a, b).astype(np.uint32)


def uniform_of(bits):
    f = ((bits >> np.uint32(9)) | np.uint32(0x3F800000)).view(F) - F(1.0)
    return np.maximum(np.finfo(F).tiny, f)  # f * (1 - tiny) + tiny == f in fp32 for f >= 2^-23, tiny for f == 0


def sample_ref(x, key, temperature=1.0, *, suppress_eos=False, eos=2, thr=None, lim=None):
    """[R][V] logits -> (drawn index per row, admissible per row, margin / bound per row)"""
    from oracle import generation_ref as G

    R, V = x.shape
    u = uniform_of(G.random_bits(key, R * V)).astype(np.float64).reshape(R, V)
    g = -np.log(-np.log(u))
    idx, ok, info = [], [], []
    for r in range(R):
        y = scaled(x[r], temperature, suppress_eos, eos)
        if thr is not None:
            y = np.where(mask_of(y, thr[r], lim[r]), y, NEG)
        s = y + g[r]
        b = EPS_F * (1 + np.abs(g[r])) + U32 * np.abs(np.where(np.isfinite(s), s, 0.0))
        o = order(s, 2)
        gap = s[o[0]] - s[o[1]] if V > 1 else np.inf
        need = b[o[0]] + (b[o[1]] if V > 1 else 0.0)
        idx.append(int(o[0]))
        ok.append(bool(gap > need))
        info.append((float(gap), float(need)))
    return np.array(idx), ok, info


# ------------------------------------------------------------------------------------------------ greedy step
def greedy_ref(top_idx, sequences, finished, cur_len, eos, pad):
    tok = np.asarray(top_idx).copy()
    fin = (np.asarray(finished) != 0) | (tok == eos)
    tok = np.where(fin, pad, tok)
    seq = np.asarray(sequences).copy()
    seq[:, cur_len] = tok
    return seq, fin.astype(np.int32), tok


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 numpy emulations of the kernels' arithmetic.  `defect` seeds the mistakes the suite has to reject; None = as designed.
def _exp32(a):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(a.astype(F)).astype(F)


def emu_lse(x, defect=None):
    """(mx, logsum) of row_lse_topk_kernel's pass 1: 256 threads, 4 x 256 chunks of 8 columns per trip, online rescale, LDS tree"""
    x = np.asarray(x, np.float64).astype(F)
    V = x.size
    nvalid = (V // 8) * 8 if defect == "no_tail" else V
    trips = -(-((V + 7) // 8) // 1024)
    pad = np.full(trips * 8192, np.nan, F)
    pad[:nvalid] = x[:nvalid]
    t = pad.reshape(trips, 4, 256, 8).transpose(0, 2, 1, 3).reshape(trips, 256, 32)  # [trip][thread][u * 8 + i]
    ok = ~np.isnan(t)
    m, s = np.full(256, NEG, F), np.zeros(256, F)
    with np.errstate(invalid="ignore"):
        for p in range(trips):
            cm = np.where(ok[p], t[p], NEG).max(1).astype(F)
            mn = np.maximum(m, cm)
            add = np.zeros(256, F)
            for j in range(32):
                add = np.where(ok[p][:, j], add + _exp32(t[p][:, j] - mn), add).astype(F)
            s = np.where(mn == NEG, F(0), s * _exp32(m - mn) + add).astype(F)
            m = mn
        o = 128
        while o:
            m1, m2 = m[:o], m[o:2 * o]
            mn = np.maximum(m1, m2)
            s = np.concatenate([np.where(mn == NEG, F(0), s[:o] * _exp32(m1 - mn) + s[o:2 * o] * _exp32(m2 - mn)).astype(F), s[o:]])
            m = np.concatenate([mn, m[o:]])
            o >>= 1
    return m[0], np.log(s[0]).astype(F)


def emu_proc(x, mx, logsum, bias, suppress_eos, eos, raw, defect=None):
    x = np.asarray(x, np.float64).astype(F)
    with np.errstate(invalid="ignore"):
        v = x if raw else ((x - mx).astype(F) - logsum).astype(F)
        v = np.where(np.isneginf(x), F(NEG), v)
        if suppress_eos and defect != "no_eos" and 0 <= eos < x.size:
            v[eos] = NEG
        return (v + F(bias)).astype(F)


def emu_lse_values(x, bias=0.0, *, suppress_eos=False, eos=2, raw=False, defect=None):
    """the fp32 processed values of one row as row_lse_topk_kernel forms them"""
    x = np.asarray(x, np.float64)
    if defect == "bias_first" and not raw:  # the running score added to the logits: the log-softmax removes it again
        mx, ls = emu_lse(x + float(F(bias)))
        return emu_proc((x + float(F(bias))), mx, ls, 0.0, suppress_eos, eos, raw)
    mx, ls = (F(0), F(0)) if raw else emu_lse(x, defect)
    return emu_proc(x, mx, ls, bias, suppress_eos, eos, raw, defect)


def emu_row_lse_topk(x, k, bias=0.0, *, defect=None, values=None, suppress_eos=False, eos=2, raw=False):
    """(values fp32, indices) of one row; raw_logits with k = 1 is the kernel's argmax branch: the first maximum of the logits"""
    v = emu_lse_values(x, bias, defect=defect, suppress_eos=suppress_eos, eos=eos, raw=raw) if values is None else values
    key = v
    if raw and k == 1:
        key = np.asarray(x, np.float64).copy()
        if suppress_eos and defect != "no_eos" and 0 <= eos < key.size:
            key[eos] = NEG
    i = order(key, k, highest_index=defect == "highest_index")
    return v[i], i


def emu_row_topk_tiles(x, part, k, bias=0.0, *, suppress_eos=False, eos=2, raw=False, defect=None):
    """row_topk_tiles_kernel: lse from the partials, tau = the kk-th largest granule maximum, the candidate granules A (above f(tau))
    and the first kk of E (equal to it), the top-k among their elements"""
    x = np.asarray(x, np.float64)
    V, nt = x.size, part.shape[0]
    tm, ts = part[:, 0].astype(F), part[:, 1].astype(F)
    mx, ls = F(0), F(0)
    if not raw:
        mx = tm.max()
        with np.errstate(invalid="ignore"):
            ls = np.log(np.where(np.isneginf(tm), F(0), ts * _exp32(tm - mx)).astype(F).sum(dtype=F)).astype(F)
    kk = k + (1 if suppress_eos and defect != "tau_k" else 0)
    srt = np.sort(tm)[::-1]
    tau = srt[kk - 1] if kk <= nt else F(NEG)
    f = lambda a: emu_proc(a, mx, ls, bias, False, eos, raw)  # noqa: E731
    ftau, fm = f(np.array([tau]))[0], f(tm)
    E = np.flatnonzero(fm == ftau)[:kk]
    A = np.flatnonzero(fm > ftau)
    cols = np.sort(np.concatenate([np.arange(g * 64, min(g * 64 + 64, V)) for g in np.concatenate([E, A])[:34]] or [np.zeros(0, int)]).astype(int))
    v = emu_proc(x, mx, ls, bias, suppress_eos, eos, raw, defect)
    o = order(v[cols], k)
    val, idx = np.full(k, NEG, F), np.full(k, NOIDX, np.int64)
    val[:o.size], idx[:o.size] = v[cols][o], cols[o]
    return val, idx


def okey(v, canon=True):
    v = np.asarray(v, F).copy()
    if canon:
        v[v == 0] = F(0.0)
    u = v.view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def okey_inv(k):
    k = np.uint32(k)
    return (np.uint32(k & np.uint32(0x7FFFFFFF)) if k & np.uint32(0x80000000) else np.uint32(~k)).view(F)


def emu_warp(x, temperature, top_k, top_p, *, suppress_eos=False, eos=2, defect=None):
    """warp_threshold_kernel on one row of stored logits: (thr, tie_limit).  The radix descent over the 32-bit keys finds the key at
    which the running weight (counts / fixed-point masses, exact integer sums) first reaches the target; == and < compare floats"""
    canon = defect != "no_canon"
    v0 = np.asarray(x, np.float64).astype(F)
    if F(temperature) != F(1.0):
        v0 = (v0 / F(temperature)).astype(F)
    if suppress_eos and 0 <= eos < v0.size:
        v0[eos] = NEG
    V, idx = v0.size, np.arange(v0.size)
    thr, lim = F(NEG), NOIDX

    def at():
        return np.where((v0 < thr) | ((v0 == thr) & (idx >= lim)), F(NEG), v0)

    for stage in (0, 1):
        if stage == 0 and (top_k <= 0 or top_k >= V):
            continue
        if stage == 1 and not F(top_p) < F(1.0):
            continue
        v = at()
        live = v > NEG
        if stage == 0:
            w, target = np.ones(V, np.int64), int(top_k)
        else:
            mx = v.max()
            w = (_exp32(v - mx) * F(1099511627776.0)).astype(np.int64)
            t = float(F(top_p)) * float(w[live].sum())
            target = int(t) + (1 if float(int(t)) < t else 0)
            target = max(target, 1)
        keys = okey(v, canon=canon)  # -0 := +0 in the key alone: every other use of v is a comparison or v - mx, which see one zero
        if not live.any():
            continue
        srt = np.argsort(keys[live], kind="stable")[::-1]
        kl, wl = keys[live][srt], w[live][srt]
        first = np.r_[True, kl[1:] != kl[:-1]]
        ks, wk = kl[first], np.add.reduceat(wl, np.flatnonzero(first))
        cum = np.cumsum(wk)
        j = int(np.searchsorted(cum, target))
        if j >= ks.size:
            continue  # fewer surviving entries than requested: nothing to cut
        need = target - (cum[j] - wk[j])
        t_new = okey_inv(ks[j])
        if stage == 0:
            n_keep = need
        else:
            m_eq = int(_exp32(np.array([t_new - mx], F))[0] * F(1099511627776.0))
            n_keep = -(-need // m_eq) if m_eq else NOIDX
        if defect == "n_keep_off":
            n_keep += 1
        eq = np.flatnonzero(v == t_new)
        new_lim = int(eq[n_keep - 1]) + 1 if 1 <= n_keep <= eq.size else NOIDX
        thr, lim = t_new, new_lim
    return float(thr), int(lim)


def emu_sample(x, key, temperature=1.0, *, suppress_eos=False, eos=2, thr=None, lim=None, defect=None):
    """sample_rows_kernel on [R][V] stored logits: the drawn index per row"""
    R, V = x.shape
    u = uniform_of(kernel_bits(key, R * V, defect)).reshape(R, V)
    with np.errstate(divide="ignore"):
        g = (-np.log((-np.log(u)).astype(F))).astype(F)
    out = []
    for r in range(R):
        v = np.asarray(x[r], np.float64).astype(F)
        if F(temperature) != F(1.0):
            v = (v / F(temperature)).astype(F)
        if thr is not None:
            v = np.where((v < F(thr[r])) | ((v == F(thr[r])) & (np.arange(V) >= lim[r])), F(NEG), v)
        if suppress_eos and 0 <= eos < V:
            v[eos] = NEG
        out.append(int(order((v + g[r]).astype(F), 1)[0]))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ thresholds for the sampling cases
def pair_of(y, keep):
    """the (thr, tie_limit) pair that stands for a warper mask over the scaled scores y ((-inf, 0x7fffffff): nothing cut)"""
    y = np.asarray(y, np.float64)
    if np.array_equal(keep, np.isfinite(y)):
        return NEG, NOIDX
    thr = y[keep].min()
    pair = thr, int(np.flatnonzero(keep & (y == thr)).max()) + 1
    assert np.array_equal(mask_of(y, *pair), keep), "a warper mask that no (thr, tie_limit) pair stands for"
    return pair


def sample_setup(x, variant):
    """dict(temperature, suppress_eos, eos, thr, lim) of a sampling variant of util_decode_cases.SAMPLE_VARIANTS: the thresholds are
    the fp64 warpers' (row 0 of topk1_topk3 keeps one token, row 1 — the signed-zero row — three)"""
    R, V = x.shape
    T, sup, ks, p = {"plain": (1.0, False, None, 1.0), "temperature_eos": (0.7, True, None, 1.0),
                     "topk1_topk3": (1.0, False, [1, 3] + [5] * (R - 2), 1.0), "topk_topp": (2.0, True, [50] * R, 0.9)}[variant]
    out = dict(temperature=T, suppress_eos=sup, eos=2, thr=None, lim=None)
    if ks is not None:
        pairs = [pair_of(y, warp_ref(y, k, p)["keep"]) for y, k in ((scaled(x[r], T, sup, 2), ks[r]) for r in range(R))]
        out["thr"], out["lim"] = np.array([q[0] for q in pairs], F), np.array([q[1] for q in pairs], np.int32)
    return out
