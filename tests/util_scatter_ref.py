"""fp64 references, derived bounds and numpy emulations for the gather / scatter conformance suite
(tests/test_scatter_conformance_{cpu,gpu}.py).  A helper module, not a conftest.

References follow include/mic_hip.h on the operands as stored; emulations (`emu_*`) restate the kernels' fp32 arithmetic in the
order csrc/elementwise.hip performs it and take a `defect` that seeds one flaw.  Three kinds of check:

  exact      pure data movement (im2col, dpatch, copy_rows, casts, row flags, the dropout mask): the bits of the reference.
  one        one fp32 operation chain then the store (mic_embed_fwd, mic_vit_assemble): with ref = a * scale + p in fp64,
             |got - ref| <= stored(U32 (|a scale| + |ref|)) — the product and the sum round once each, or once together when the
             compiler contracts them; the bound holds either way.
  sums       with k the longest chain of fp32 adds an element passes through (written beside each case):
             |got - ref| <= gamma_k(k) sum |terms| + U32 |start|.
             gamma_k(k) = 2 k 2^-24 is twice the first-order bound of k sequential adds of the terms; the start value takes part
             in the A atomic adds that reach the element, each rounding at most U32 (|start| + sum |terms|), so the start's share
             is A U32 |start|, of which (A - 1) U32 |start| has to come out of the unused half of gamma_k: this needs
             (A - 1) |start| <= k sum |terms|, which A <= k and |start| <= sum |terms| give (`atomic_bound` asserts the latter; the
             cases' start values are drawn that way, util_scatter_cases.start_values).
The deterministic scatter is additionally compared bit for bit with `emu_det`, the documented order."""
from __future__ import annotations

import numpy as np

from util_gemm_ref import U32, gamma_k, round_to
from util_rowop_ref import stored

F32 = np.float32


def _f32(x):
    return np.asarray(x, np.float64).astype(F32)


def one_rounding_bound(a_scaled, ref, dtype):
    return stored(None, dtype)(ref, U32 * (np.abs(a_scaled) + np.abs(ref)))


def atomic_bound(k, abs_sum, start=None, atomics=None):
    """gamma_k(k) sum |terms| + U32 |start|; `atomics`: how many atomic adds reach an element (default: as many as k).  Asserts the
    condition of the module docstring, (A - 1) |start| <= k sum |terms|"""
    if start is None:
        return gamma_k(k) * abs_sum + 1e-300
    A = k if atomics is None else atomics
    assert ((A - 1) * np.abs(start) <= k * abs_sum).all(), "a start value too large for the sum of the terms: the bound is not one"
    return gamma_k(k) * abs_sum + U32 * np.abs(start) + 1e-300


# ------------------------------------------------------------------------------------------------ im2col
def im2col_ref(px, B, img, ps, trunc, dtype, defect=None):
    """patches[(b g + pi) g + pj][(u ps + v) 3 + c] = pixels[b][pi ps + u][pj ps + v][c], as stored (fp32 -> dtype, RNE).  trunc: the
    value of the cast through int32, i.e. rounding toward zero (its zero is +0 or -0: equal as values)"""
    g = img // ps
    x = np.trunc(px) if trunc else px
    p = x.reshape(B, g, ps, g, ps, 3).transpose(0, 1, 3, 2, 4, 5)      # b, pi, pj, u, v, c
    if defect == "k_order_cuv":
        p = p.transpose(0, 1, 2, 5, 3, 4)
    return round_to(p.reshape(B * g * g, ps * ps * 3), dtype)


# ------------------------------------------------------------------------------------------------ ViT assembly
def vit_assemble_ref(patch, cls, pos, B, S, dtype, defect=None):
    """x[b, 0] = cls + pos[0]; x[b, 1 + p] = patch[b (S - 1) + p] + pos[1 + p]: (ref [B S][W], bound)"""
    W = patch.shape[1]
    a = np.empty((B, S, W))
    a[:, 0] = cls
    if defect == "patch_row_bS":   # b * S where b * (S - 1) is right
        idx = (np.arange(B)[:, None] * S + np.arange(S - 1)[None, :]) % patch.shape[0]
        a[:, 1:] = patch[idx]
    else:
        a[:, 1:] = patch.reshape(B, S - 1, W)
    ref = (a + pos[None]).reshape(B * S, W)
    return ref, one_rounding_bound(a.reshape(B * S, W), ref, dtype)


def emu_vit_assemble(patch, cls, pos, B, S, dtype, defect=None):
    W = patch.shape[1]
    a = np.empty((B, S, W), F32)
    a[:, 0] = _f32(cls)
    if defect == "patch_row_bS":
        idx = (np.arange(B)[:, None] * S + np.arange(S - 1)[None, :]) % patch.shape[0]
        a[:, 1:] = _f32(patch)[idx]
    else:
        a[:, 1:] = _f32(patch).reshape(B, S - 1, W)
    return round_to((a + _f32(pos)[None]).astype(np.float64).reshape(B * S, W), dtype)


def vit_bwd_ref(dx, dpos0, dcls0, k):
    """dx [B][S][W]: dpatch (exact), (dpos, bound), (dcls, bound)"""
    B, S, W = dx.shape
    a = np.abs(dx).sum(0)
    return (dx[:, 1:].reshape(B * (S - 1), W), (dpos0 + dx.sum(0), atomic_bound(k, a, dpos0)),
            (dcls0 + dx[:, 0].sum(0), atomic_bound(k, a[0], dcls0)))


def emu_vit_bwd(dx, dpos0, dcls0, slices, defect=None):
    """slices 0: the element kernel (one sum over b, one atomic); else the batch cut into `slices` pieces of ceil(B / slices), each
    summed from 0 in order, the pieces added to the start value in slice order (one of the orders the atomics can take)"""
    B, S, W = dx.shape
    x = _f32(dx)
    per = B if not slices else -(-B // slices)
    dpos, dcls = _f32(dpos0).copy(), _f32(dcls0).copy()
    for b0 in range(0, max(slices, 1) * per, per):
        b1 = min(B, b0 + per)
        acc = np.zeros((S, W), F32)
        for b in range(b0, b1):
            acc = acc + x[b]
        dpos = dpos + acc
        dcls = dcls + (acc.sum(0, dtype=F32) if defect == "dcls_all_s" else acc[0])
    if defect == "dpatch_bS":
        dp = np.zeros((B * (S - 1), W))
        for b in range(B):
            for s in range(1, S):
                dp[(b * S + s - 1) % (B * (S - 1))] = dx[b, s]
    else:
        dp = dx[:, 1:].reshape(B * (S - 1), W)
    return dp, dpos.astype(np.float64), dcls.astype(np.float64)


# ------------------------------------------------------------------------------------------------ token embedding
def embed_fwd_ref(ids, pos, table, ptab, scale, dtype):
    sc = float(F32(scale))
    a = table[ids] * sc
    ref = a + ptab[pos + 2]
    return ref, one_rounding_bound(a, ref, dtype)


def emu_embed_fwd(ids, pos, table, ptab, scale, dtype, contract=False, defect=None):
    off = 0 if defect == "no_plus2" else 2
    p = np.nan_to_num(ptab, nan=1e30)[pos + off] if defect else ptab[pos + off]
    if contract:   # one rounding: the product is exact in fp64
        v = (table[ids] * float(F32(scale)) + p).astype(F32)
    else:
        v = _f32(table[ids]) * F32(scale) + _f32(p)
    return round_to(v.astype(np.float64), dtype)


def embed_bwd_ref(ids, pos, dh, scale, V, P2, dt0=None, dp0=None):
    """(dtable, bound), (dpos, bound): k = occurrences + 1 for dtable (dh * scale rounds, then one atomic per occurrence), the
    occurrences for dpos"""
    sc = float(F32(scale))
    W = dh.shape[1]
    out = []
    for idx, n, terms, start, extra in ((ids, V, dh * sc, dt0, 1), (pos + 2, P2, dh, dp0, 0)):
        s, a = np.zeros((n, W)), np.zeros((n, W))
        np.add.at(s, idx, terms)
        np.add.at(a, idx, np.abs(terms))
        cnt = np.bincount(idx, minlength=n)[:, None]
        st = np.zeros((n, W)) if start is None else start
        out.append((st + s, atomic_bound(cnt + extra, a, st, cnt)))
    return out


def emu_embed_bwd(ids, pos, dh, scale, V, P2, dt0=None, dp0=None, defect=None):
    """fp32 atomics in row order (one of the orders they can take)"""
    W = dh.shape[1]
    g = _f32(dh)
    dt = np.zeros((V, W), F32) if dt0 is None else _f32(dt0).copy()
    dp = np.zeros((P2, W), F32) if dp0 is None else _f32(dp0).copy()
    np.add.at(dt, ids, g * F32(scale))
    np.add.at(dp, pos + (0 if defect == "no_plus2" else 2), g * F32(scale) if defect == "scale_on_dpos" else g)
    return dt.astype(np.float64), dp.astype(np.float64)


# ------------------------------------------------------------------------------------------------ deterministic scatter
def det_ref(ids, dh, scale, base):
    """fp64 dtable and the bound gamma_k(count + 2) scale sum |dh| + U32 |base|: at most count - 1 adds of the rows round (an add
    to 0 is exact), then the product with scale and the add to the table row"""
    sc = float(F32(scale))
    ok = ids >= 0
    s, a = np.zeros_like(base), np.zeros_like(base)
    np.add.at(s, ids[ok], dh[ok])
    np.add.at(a, ids[ok], np.abs(dh[ok]))
    cnt = np.bincount(ids[ok], minlength=base.shape[0])[:, None]
    return base + s * sc, gamma_k(1) * (cnt + 2) * abs(sc) * a + U32 * np.abs(base) + 1e-300


def _seq_sum(rows):
    """0 + r0 + r1 + ... in fp32, in order"""
    return np.cumsum(rows, axis=0, dtype=F32)[-1] if len(rows) else 0.0


def emu_det(ids, dh, scale, base, defect=None):
    """the documented order in fp32 (exact for a power-of-two scale, where contracting t * scale + base changes nothing):
         1 or 2 occurrences:  base + (dh[first] (+ dh[last])) * scale
         more:                sixteen partial rows, each summed from 0 in index order — the occurrences in bitmap word w = i >> 5 go
                              to group (w ^ (w >> 4)) % 16 — the partials summed from 0 in group order, times scale, added to base.
       defects: 'mod16' (group w % 16), 'single_twice' (a single occurrence handled as first + last), 'no_tail' (the scan stops at
       n - n % 4), 'no_block2' (columns from 1024 on of ids with more than two occurrences are not written)"""
    out = _f32(base).copy()
    x = _f32(np.nan_to_num(dh))
    sc = F32(scale)
    n = ids.shape[0]
    order = np.argsort(ids, kind="stable")          # ascending positions inside one id
    sid = ids[order]
    lo = np.searchsorted(sid, 0)
    uniq, start, cnt = np.unique(sid[lo:], return_index=True, return_counts=True)
    first, last = order[lo + start], order[lo + start + cnt - 1]
    one, two = cnt == 1, cnt == 2
    if defect == "single_twice":
        one, two = np.zeros_like(one), one | two
    out[uniq[one]] = out[uniq[one]] + x[first[one]] * sc
    out[uniq[two]] = out[uniq[two]] + (x[first[two]] + x[last[two]]) * sc
    for u, b0, c in zip(uniq[cnt > 2], (lo + start)[cnt > 2], cnt[cnt > 2]):
        occ = order[b0:b0 + c]
        if defect == "no_tail":
            occ = occ[occ < n - n % 4]
        w = occ >> 5
        g = (w % 16) if defect == "mod16" else ((w ^ (w >> 4)) % 16)
        t = np.zeros(x.shape[1], F32)
        for q in range(16):
            t = t + _seq_sum(x[occ[g == q]])
        new = out[u] + t * sc
        if defect == "no_block2":
            new[1024:] = out[u][1024:]
        out[u] = new
    return out


# ------------------------------------------------------------------------------------------------ column sums
def colsum_ref(x, k, start=None):
    a = np.abs(x).sum(0)
    return x.sum(0) + (0.0 if start is None else start), atomic_bound(k, a, start)


def emu_colsum(x, plan, start=None, defect=None, scale=None):
    """the lane / LDS / grid split of colsum_kernel: a block = 256 columns x one slice of rows_per rows; row lane rl sums rows
    r0 + rl, r0 + rl + 8, ... from 0; the eight lanes are summed from 0 in lane order; the slices reach the output in slice order
    (one of the orders the atomics can take).  scale: colsum_q8's product with scale_inv in front of the atomic"""
    gx, gy, rows_per, _ = plan
    rows, cols = x.shape
    v = _f32(x)
    out = np.zeros(cols, F32) if start is None else _f32(start).copy()
    for by in range(gy - (defect == "no_last_slice")):
        r0, r1 = by * rows_per, min(rows, (by + 1) * rows_per)
        s = np.zeros(cols, F32)
        for rl in range(8):
            s = s + (_seq_sum(v[r0 + rl:r1:8]) if r0 + rl < r1 else F32(0))
        if defect == "no_partial_chunk":
            s[cols // 8 * 8:] = 0
        out = out + (s if scale is None else s * F32(scale))
    return out.astype(np.float64)


def _q8_tables():
    """value of every byte of the two OCP 8-bit formats, written out from the definition: e4m3fn (bias 7, no infinity, S.1111.111 the
    only NaN, subnormals m / 8 * 2^-6) and e5m2 (bias 15, IEEE-like: exponent 31 is inf / NaN, subnormals m / 4 * 2^-14)"""
    t = {"e4m3": np.zeros(256), "e5m2": np.zeros(256)}
    for b in range(256):
        s = -1.0 if b & 0x80 else 1.0
        e, m = (b >> 3) & 0xF, b & 0x7
        t["e4m3"][b] = np.nan if (e == 15 and m == 7) else s * (m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
        e, m = (b >> 2) & 0x1F, b & 0x3
        t["e5m2"][b] = (s * np.inf if m == 0 else np.nan) if e == 31 else s * (m / 4 * 2.0 ** -14 if e == 0 else (1 + m / 4) * 2.0 ** (e - 15))
    return t


Q8_TABLE = _q8_tables()


def q8_decode(b, fmt, defect=None):
    if defect == "as_e4m3":
        fmt = "e4m3"
    v = Q8_TABLE[fmt][b]
    if defect == "flush_subnormals":
        v = np.where((b & (0x78 if fmt == "e4m3" else 0x7C)) == 0, 0.0, v)
    return v


def colsum_q8_ref(b, fmt, scale_inv, k, start):
    """out = start + scale_inv * column sums of the decoded bytes"""
    x = q8_decode(b, fmt) * float(F32(scale_inv))
    return colsum_ref(x, k, start)


# ------------------------------------------------------------------------------------------------ casts
def cast_expected_bits(src_bits, src, dst, defect=None):
    """the destination's bit patterns (uint32 / uint16) and a mask of the NaNs, which only have to stay NaN"""
    if src == "bf16":
        nan = ((src_bits & 0x7F80) == 0x7F80) & ((src_bits & 0x7F) != 0)
        return (src_bits.astype(np.uint32) << 16 if dst == "f32" else src_bits), nan
    f = src_bits.view(F32)
    nan = np.isnan(f)
    if dst == "f32":
        return src_bits, nan
    if defect == "truncate":
        return (src_bits >> 16).astype(np.uint16), nan
    with np.errstate(invalid="ignore"):
        r = round_to(f.astype(np.float64), "bf16").astype(F32)   # RNE, infinities kept
    return (r.view(np.uint32) >> 16).astype(np.uint16), nan


# ------------------------------------------------------------------------------------------------ slabs
def sum_slabs_ref(x, dtype):
    """x [n][rows][cols]: (fp64 sum, bound through the store)"""
    s = x.sum(0)
    return s, stored(None, dtype)(s, gamma_k(x.shape[0]) * np.abs(x).sum(0))


def emu_sum_slabs(x, dtype, defect=None):
    """0 + s0 + s1 + ... in slab order, one rounding to the output type"""
    v = _f32(x)
    if defect == "pairwise":
        while v.shape[0] > 1:
            h = v.shape[0] // 2
            v = np.concatenate([v[:h] + v[h:2 * h], v[2 * h:]], 0)
        acc = v[0]
    else:
        acc = np.zeros(v.shape[1:], F32)
        for s in v:
            acc = acc + s
    return round_to(acc.astype(np.float64), dtype)


# ------------------------------------------------------------------------------------------------ label terms
def label_terms_ref(labels, coef, E, h, dE0):
    """dx_slab (fp64, bound U32 |ref|: one product), dE (fp64, bound with k = rows of the label whose coef != 0, + 1 for the product)"""
    live = coef != 0
    dx = np.where(live[:, None], coef[:, None] * np.nan_to_num(E[labels]), 0.0)
    terms = coef[live, None] * h[live]
    s, a = np.zeros_like(dE0), np.zeros_like(dE0)
    np.add.at(s, labels[live], terms)
    np.add.at(a, labels[live], np.abs(terms))
    cnt = np.bincount(labels[live], minlength=dE0.shape[0])[:, None]
    return dx, U32 * np.abs(dx), dE0 + s, atomic_bound(cnt + 1, a, dE0, cnt)


def emu_label_terms(labels, coef, E, h, dE0, defect=None):
    live = (coef != 0) | (defect == "zero_coef_adds")
    c = _f32(coef)
    dx = np.where((coef != 0)[:, None], c[:, None] * _f32(np.nan_to_num(E))[labels], F32(0)).astype(F32)
    dE = _f32(dE0).copy()
    hh = _f32(np.nan_to_num(h, nan=1.0))
    cc = np.where(coef != 0, c, F32(1e-3)) if defect == "zero_coef_adds" else c
    np.add.at(dE, labels[live], cc[live, None] * hh[live])
    return dx, dE.astype(np.float64)
