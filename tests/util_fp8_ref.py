"""Reference of the fp8 emission contract (csrc/fp8.hip, common.h Q8Out: the quantiser and the producers that write fp8 bytes
themselves) for tests/test_fp8_conformance_{cpu,gpu}.py, and numpy emulations of the emitters' arithmetic with seeded defects for
the check on the checker.  A helper module, not a conftest.

The encoder `q8_encode` uses nothing but the value tables util_scatter_ref.Q8_TABLE writes out from the OCP definition: the byte
whose value is nearest, ties to the even mantissa (= the even byte), saturating at +-FMAX, the sign kept (so -0.0 and every
negative value that rounds to zero give 0x80).

The emission contract, `emit_ref(v, amax_old, fmt)` on a tensor v of bf16 values:
    scale    = min(fl32(FMAX / amax_old), FLT_MAX) if amax_old > 0 else 1         (fl32: one correctly rounded fp32 operation)
    state[1] = fl32(amax_old / FMAX) if amax_old > 0 else 1
    byte     = q8_encode(clamp(fl32(v * scale), +-FMAX))
    recorded amax = max |v| over the valid region, exactly
Current scaling (mic_fp8_amax, then mic_fp8_quantize) is the same function with amax_old = max |v|.
The clamp of the scale at FLT_MAX is what keeps 0 * scale a zero for 0 < amax_old < FMAX / FLT_MAX (1.3e-36 for e4m3, 1.7e-34
for e5m2: normal bf16 values), where FMAX / amax_old overflows.

`emit_interval(y, bound, amax_old, fmt)` is for emitters that leave no bf16 copy: the value the kernel quantises may be any bf16
value in [y - bound, y + bound]; the encoder and the scaling are monotone, so the admissible bytes are those from
Q(bf16_down(y - bound)) to Q(bf16_up(y + bound)) in the order of their values.  store='f32': the kernel quantises an fp32 value
without the bf16 rounding (mic_ce_bwd_q8), the ends are y -+ bound rounded outward to fp32.

Bytes compare exactly, except that 0x00 and 0x80 both count as zero where the reference byte is a zero."""
from __future__ import annotations

import numpy as np

import util_rowop_ref as RR
from util_gemm_ref import round_bf16
from util_scatter_ref import Q8_TABLE

F32 = np.float32
FMAX = {"e4m3": 448.0, "e5m2": 57344.0}
FLT_MAX = float(np.finfo(F32).max)
NAN_BYTE = {"e4m3": 0x7F, "e5m2": 0x7E}
PARTIALS = 1024
FMTS = ("e4m3", "e5m2")


def _grid(fmt):
    """the non-negative finite values in byte order: byte b < len has value grid[b]"""
    t = Q8_TABLE[fmt][:128]
    n = int(np.isfinite(t).sum())
    g = t[:n]
    assert np.isfinite(g).all() and (np.diff(g) > 0).all() and g[-1] == FMAX[fmt] and not np.isfinite(t[n:]).any()
    return g


GRID = {f: _grid(f) for f in FMTS}


def q8_encode(t32, fmt, defect=None):
    """float32 -> fp8 byte.  defects: 'fnuz' (the exponent bias of the FNUZ encodings: one more), 'truncate' (toward zero),
    'flush_subnormals' (results with a zero exponent field become zero), 'no_saturate' (beyond FMAX: inf / NaN as an IEEE-style
    conversion gives)"""
    x = np.asarray(t32, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.abs(x.astype(np.float64)) * (2.0 if defect == "fnuz" else 1.0)
    g = GRID[fmt]
    n = len(g)
    hi = np.minimum(np.searchsorted(g, np.where(np.isnan(a), 0.0, a), side="left"), n - 1)
    lo = np.maximum(hi - 1, 0)
    with np.errstate(invalid="ignore"):
        dlo, dhi = a - g[lo], g[hi] - a
        pick_hi = (dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)) | (a >= g[n - 1])
        if defect == "truncate":
            pick_hi = (a >= g[hi])
    b = np.where(pick_hi, hi, lo).astype(np.uint8)
    if defect == "flush_subnormals":
        b = np.where(b < (8 if fmt == "e4m3" else 4), 0, b).astype(np.uint8)
    if defect == "no_saturate":
        half = (g[-1] - g[-2]) / 2
        b = np.where(a >= g[-1] + half, NAN_BYTE[fmt] if fmt == "e4m3" else 0x7C, b).astype(np.uint8)
    b = np.where(np.isnan(a), NAN_BYTE[fmt], b).astype(np.uint8)
    return (b | np.where(np.signbit(x), 0x80, 0).astype(np.uint8)).astype(np.uint8)


def q8_brute(t32, fmt):
    """the same by a search over all 256 table entries: the nearest finite value, ties to the even byte, the sign of the input"""
    x = np.asarray(t32, F32).astype(np.float64).reshape(-1)
    t = Q8_TABLE[fmt]
    out = np.empty(x.size, np.uint8)
    cand = np.array([b for b in range(256) if np.isfinite(t[b])])
    for s in range(0, x.size, 8192):
        xs = x[s:s + 8192]
        ok = (np.signbit(t[cand])[None, :] == np.signbit(xs)[:, None])
        d = np.where(ok, np.abs(xs[:, None] - t[cand][None, :]), np.inf)
        best = d.min(1, keepdims=True)
        tie = (d == best)
        even = tie & (cand % 2 == 0)[None, :]
        use = np.where(even.any(1, keepdims=True), even, tie)
        out[s:s + 8192] = cand[use.argmax(1)]
    return out.reshape(np.shape(t32))


def order(b):
    """bytes -> integers ordered as the byte values are (both zeros 0; NaN / inf bytes beyond every finite one)"""
    b = np.asarray(b, np.uint8).astype(np.int64)
    return np.where(b & 0x80, -(b & 0x7F), b & 0x7F)


def is_finite_byte(b, fmt):
    return (np.asarray(b, np.uint8) & 0x7F) < len(GRID[fmt])


# ------------------------------------------------------------------------------------------------ the contract
def scale_of(amax_old, fmt, defect=None):
    """(scale, state[1]) as fp32 scalars"""
    fm, a = F32(FMAX[fmt]), F32(amax_old)
    if not a > 0:
        return F32(1), F32(1)
    with np.errstate(over="ignore", divide="ignore"):
        sc = F32(fm / a)
        if defect != "inf_scale":
            sc = min(sc, F32(FLT_MAX))
        if defect == "scale_inverted":
            sc = F32(a / fm)
    return sc, F32(a / fm)


def quantise(v, scale, fmt, defect=None):
    """bytes of fp32 values v under an fp32 scale.  defect 'no_clamp' plus those of q8_encode"""
    fm = F32(FMAX[fmt])
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = (np.asarray(v, F32) * F32(scale)).astype(F32)
    if defect == "no_clamp":
        return q8_encode(t, fmt, "no_saturate")
    with np.errstate(invalid="ignore"):
        t = np.minimum(np.maximum(t, -fm), fm)   # (numpy's minimum / maximum pass a NaN on: NaN is outside the checked domain)
    return q8_encode(t, fmt, defect)


def emit_ref(v, amax_old, fmt):
    """v: bf16 values (any float array).  -> (bytes, state[1], recorded amax) ; amax_old None: current scaling"""
    v = np.asarray(v, F32)
    amax = F32(np.abs(v).max()) if v.size else F32(0)
    sc, sinv = scale_of(amax if amax_old is None else amax_old, fmt)
    return quantise(v, sc, fmt), sinv, amax


def _bf16_key(v):
    b = (np.asarray(v, F32).view(np.uint32) >> 16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def _bf16_of_key(k):
    k = np.clip(k, -0x7F7F, 0x7F7F)
    b = (np.where(k < 0, 0x8000 | (-k), k).astype(np.uint32) << 16).astype(np.uint32)
    return b.view(F32).astype(np.float64)


def bf16_down(x):
    """the largest bf16 value <= x (fp64 in, fp64 out)"""
    x = np.asarray(x, np.float64)
    r = round_bf16(np.clip(x, -3.3e38, 3.3e38))
    return np.where(r <= x, r, _bf16_of_key(_bf16_key(r) - 1))


def bf16_up(x):
    x = np.asarray(x, np.float64)
    r = round_bf16(np.clip(x, -3.3e38, 3.3e38))
    return np.where(r >= x, r, _bf16_of_key(_bf16_key(r) + 1))


def f32_down(x):
    x = np.asarray(x, np.float64)
    r = x.astype(F32)
    return np.where(r.astype(np.float64) <= x, r, np.nextafter(r, F32(-np.inf))).astype(F32)


def f32_up(x):
    x = np.asarray(x, np.float64)
    r = x.astype(F32)
    return np.where(r.astype(np.float64) >= x, r, np.nextafter(r, F32(np.inf))).astype(F32)


def emit_interval(y64, bound, amax_old, fmt, store="bf16"):
    """-> (lowest admissible byte, highest admissible byte, nominal byte Q(store(y)))"""
    y, e = np.asarray(y64, np.float64), np.asarray(bound, np.float64)
    assert (e >= 0).all()
    sc, _ = scale_of(amax_old, fmt)
    if store == "bf16":
        lo, hi, nom = bf16_down(y - e), bf16_up(y + e), round_bf16(y)
    else:
        lo, hi, nom = f32_down(y - e), f32_up(y + e), y.astype(F32)
    return quantise(lo, sc, fmt), quantise(hi, sc, fmt), quantise(nom, sc, fmt)


# ------------------------------------------------------------------------------------------------ the checks
def check_bytes(got, ref, what, fmt=None):
    """exact, both zero bytes equal where the reference byte is a zero"""
    got, ref = np.asarray(got, np.uint8), np.asarray(ref, np.uint8)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bad = (got != ref) & ~(((ref & 0x7F) == 0) & ((got & 0x7F) == 0))
    print(f"[conformance] {what}: {got.size - int(bad.sum())} of {got.size} bytes equal")
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: byte {got[i]:#04x} != reference {ref[i]:#04x} at {i} ({int(bad.sum())} of {got.size} differ)")


def check_interval(got, lo, hi, nominal, what, fmt):
    """every byte between the ends of its interval (in value order) and finite; prints and returns the share that differs from the
    nominal byte"""
    got = np.asarray(got, np.uint8)
    assert got.shape == np.shape(lo), f"{what}: shape"
    og, bad = order(got), ~is_finite_byte(got, fmt)
    bad |= (og < order(lo)) | (og > order(hi))
    share = float((og != order(nominal)).mean()) if got.size else 0.0
    wide = float((order(lo) != order(hi)).mean()) if got.size else 0.0
    print(f"[conformance] {what}: share off nominal {share:.3g} over {got.size} bytes (intervals of more than one byte: {wide:.3g})")
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: byte {got[i]:#04x} outside [{np.asarray(lo)[i]:#04x}, {np.asarray(hi)[i]:#04x}] at {i} "
                             f"({int(bad.sum())} of {got.size} outside)")
    return share


def check_state(got_state1, got_amax, ref_state1, ref_amax, what):
    assert F32(got_state1) == F32(ref_state1), f"{what}: state[1] {got_state1!r} != {ref_state1!r}"
    assert F32(got_amax) == F32(ref_amax), f"{what}: recorded amax {got_amax!r} != {ref_amax!r}"
    print(f"[conformance] {what}: state[1] and the recorded amax equal")


def check_table(table, v_valid, what):
    """the partial-maximum table of one pass: its maximum is max |v| exactly, every entry is 0 or the |value| of an element"""
    t = np.asarray(table, F32)
    a = np.abs(np.asarray(v_valid, F32))
    amax = a.max() if a.size else F32(0)
    assert t.shape == (PARTIALS,) and (t >= 0).all(), f"{what}: the table holds a negative entry or a NaN"
    assert t.max() == amax, f"{what}: table maximum {t.max()!r} != max |v| {amax!r}"
    assert np.isin(t[t > 0], a).all(), f"{what}: a table entry is no |value| of the tensor"
    print(f"[conformance] {what}: partial table maximum equal ({int((t > 0).sum())} slots used)")


def amax_window(y64, bound):
    """[bf16_down(max|y| - e), bf16_up(max|y| + e)] with e the bound at the element of largest |y|"""
    y, e = np.abs(np.asarray(y64, np.float64)).reshape(-1), np.asarray(bound, np.float64).reshape(-1)
    i = int(np.argmax(y))
    return float(bf16_down(y[i] - e[i])), float(bf16_up(y[i] + e[i]))


def check_amax_window(got, y64, bound, what):
    lo, hi = amax_window(y64, bound)
    g = float(got)
    print(f"[conformance] {what}: recorded amax {g!r} in [{lo!r}, {hi!r}]")
    assert lo <= g <= hi and float(round_bf16(g)) == g, f"{what}: recorded amax {g!r} outside [{lo!r}, {hi!r}] or no bf16 value"


# ------------------------------------------------------------------------------------------------ the quantiser, whole outputs
CANARY8 = 0xA5


def quant_expect(src, rows, cols, rows_pad, fmt, amax_old):
    """src: the source allocation [>= rows][ld >= cols] of bf16 values.  -> dict(q [rows][cols], qT [cols][rows_pad] with zero pad,
    state0, state1, amax)"""
    v = np.asarray(src, F32)[:rows, :cols]
    b, sinv, amax = emit_ref(v, amax_old, fmt)
    rp = max(rows_pad, rows)
    qT = np.zeros((cols, rp), np.uint8)
    qT[:, :rows] = b.T
    return dict(q=b, qT=qT, state0=amax if amax_old is None else F32(amax_old), state1=sinv, amax=amax, v=v)


def check_quant(exp, got, what, fmt):
    """got: dict(q=None | [rows][cols], qT=None | [cols][rows_pad], state=[2], table=None | [1024])"""
    if got.get("q") is not None:
        check_bytes(got["q"], exp["q"], f"quantize/{fmt} q: {what}")
    if got.get("qT") is not None:
        rows = exp["q"].shape[0]
        assert not np.asarray(got["qT"])[:, rows:].any(), f"{what}: the pad columns of qT are not zero bytes"
        check_bytes(got["qT"], exp["qT"], f"quantize/{fmt} qT: {what}")
    st = np.asarray(got["state"], F32)
    assert st[0] == exp["state0"], f"{what}: state[0] {st[0]!r} != {exp['state0']!r}"
    assert st[1] == exp["state1"], f"{what}: state[1] {st[1]!r} != {exp['state1']!r}"
    print(f"[conformance] quantize/{fmt} state: {what}: equal")
    if got.get("table") is not None:
        check_table(got["table"], exp["v"], f"quantize/{fmt} table: {what}")


def emu_quantize(src, rows, cols, rows_pad, fmt, amax_old, defect=None):
    """mic_fp8_amax (amax_old None) + mic_fp8_quantize on the source allocation: 128 x 64 tiles, one table slot per tile
    (tile index & 1023).  defects: those of q8_encode / quantise / scale_of, 'no_fabs', 'amax_over_padding', 'qT_pad_canary',
    'no_wrap' (tiles from 1024 on drop their table write), 'state1_new' (state[1] from this pass's amax)"""
    full = np.asarray(src, F32)
    v = full[:rows, :cols]
    seen = full if defect == "amax_over_padding" else v
    amax = F32(seen.max() if defect == "no_fabs" else np.abs(seen).max())
    a_old = amax if amax_old is None else F32(amax_old)
    sc, sinv = scale_of(a_old, fmt, defect)
    if defect == "state1_new":
        sinv = scale_of(amax, fmt)[1]
    b = quantise(v, sc, fmt, defect)
    rp = max(rows_pad, rows)
    qT = np.full((cols, rp), CANARY8 if defect == "qT_pad_canary" else 0, np.uint8)
    qT[:, :rows] = b.T
    table = None
    if amax_old is not None:
        table = np.zeros(PARTIALS, F32)
        tc = -(-cols // 64)
        pad = np.zeros((-(-rows // 128) * 128, tc * 64), F32)
        pad[:rows, :cols] = np.abs(seen[:rows, :cols]) if defect != "no_fabs" else np.maximum(v, 0)
        tm = pad.reshape(-1, 128, tc, 64).max((1, 3)).reshape(-1)
        idx = np.arange(tm.size)
        keep = idx < PARTIALS if defect == "no_wrap" else np.ones(tm.size, bool)
        np.maximum.at(table, idx[keep] & (PARTIALS - 1), tm[keep])
        if defect == "amax_over_padding":
            table[0] = max(table[0], np.abs(full).max())
    return dict(q=b, qT=qT, state=np.array([a_old, sinv], F32), table=table)


def emu_roll(state, partials, defect=None):
    """mic_fp8_roll_amax on state [slots][stride] and partials [slots][1024] (copies).  defect 'no_clear'"""
    st, p = np.array(state, F32), np.array(partials, F32)
    m = p.max(1)
    st[:, 0] = np.where(m > 0, m, st[:, 0])
    if defect != "no_clear":
        p[:] = 0
    return st, p


def check_roll(state0, partials0, state1, partials1, what):
    """slot i: state[i][0] = max of its table if that is > 0, else unchanged; every other entry of state unchanged; the tables zero"""
    s0, p0, s1, p1 = (np.asarray(t, F32) for t in (state0, partials0, state1, partials1))
    m = p0.max(1)
    want = s0.copy()
    want[:, 0] = np.where(m > 0, m, s0[:, 0])
    assert np.array_equal(s1.view(np.uint32), want.view(np.uint32)), f"{what}: state after the roll"
    assert not p1.view(np.uint32).any(), f"{what}: the tables are not cleared"
    print(f"[conformance] roll_amax: {what}: {s0.shape[0]} slots equal, tables cleared")


# ------------------------------------------------------------------------------------------------ fused emitters
def emu_emit(v32, amax_old, fmt, defect=None, valid=None):
    """a fused emitter's tail on the fp32 results v32 of its producer: round to bf16, record max |x|, scale, clamp, encode.
    -> (bytes, state[1], recorded amax).  defects: 'no_bf16_rounding', 'no_fabs', 'state1_new', 'no_wrap' is the caller's"""
    v = np.asarray(v32, F32)
    r = v if defect == "no_bf16_rounding" else round_bf16(v.astype(np.float64)).astype(F32)
    seen = r if valid is None else r[valid]
    amax = F32(seen.max() if defect == "no_fabs" else np.abs(seen).max()) if seen.size else F32(0)
    sc, sinv = scale_of(amax_old, fmt, defect)
    if defect == "state1_new":
        sinv = scale_of(amax, fmt)[1]
    return quantise(r, sc, fmt, defect), sinv, amax


def ce_q8_ref(x, V, labels, mask, ls, lse):
    """the fp64 gradient g = mask (softmax - soft_label) in [-1, 1] of mic_ce_bwd_q8 with the bound util_rowop_ref.ce_bwd_ref gives for
    the fp32 gradient before storage rounding (its dtype 'f32' bound: one fp32 rounding of the value, here the product with FMAX),
    [rows][Vpad]; a label outside [0, V) matches no column: every column of that row has the soft label `low`"""
    x = np.asarray(x, np.float64)
    labels = np.asarray(labels)
    out = (labels < 0) | (labels >= V)
    g, e = RR.ce_bwd_ref(x, V, np.where(out, 0, labels), mask, ls, lse, 1.0, 1.0, "f32")
    if out.any():   # column 0 of those rows from a run whose label is column 1
        g1, e1 = RR.ce_bwd_ref(x[out], V, np.ones(int(out.sum()), np.int64), np.asarray(mask)[out], ls, np.asarray(lse)[out], 1.0, 1.0, "f32")
        g[out, 0], e[out, 0] = g1[:, 0], e1[:, 0]
    return g, e


def emu_ce_bwd_q8(x, V, labels, mask, ls, lse, denom, loss_scale, fmt, label_coef=False, colsum0=None, defect=None):
    """ce_bwd_q8_kernel: g = w (expf(x - lse) - soft) in fp32 with w = mask ? 1 : 0, byte = Q(clamp(g FMAX)); column sums of g per
    256-row block (16 rows per wave in order, the four waves pairwise, the blocks in order), times loss_scale / denom.
    -> dict(q [rows][Vpad], state [2], coef [rows] | None, colsum [Vpad] | None).  defects: q8_encode's, 'no_clamp',
    'label_written' (label_coef mode still writes the label's byte), 'pad_cols' (columns V .. Vpad not zeroed)"""
    x = np.asarray(x, F32)
    R, Vp = x.shape
    fm = F32(FMAX[fmt])
    lsf = F32(ls)
    conf, low = F32(1) - lsf, (F32(lsf / F32(V - 1)) if ls > 0 else F32(0))
    w = np.where(np.asarray(mask) != 0, F32(1), F32(0))[:, None]
    lab = np.asarray(labels)
    soft = np.full((R, Vp), low, F32)
    ok = (lab >= 0) & (lab < V)
    soft[np.arange(R)[ok], lab[ok]] = conf
    g = (w * (RR._expf(x - np.asarray(lse, F32)[:, None]) - soft).astype(F32)).astype(F32)
    if defect != "pad_cols":
        g[:, V:] = 0
    inv = F32(F32(loss_scale) / F32(denom))
    o = g.copy()
    coef = None
    if label_coef:
        coef = np.zeros(R, F32)
        coef[ok] = (g[np.arange(R)[ok], lab[ok]] * inv).astype(F32)
        if defect != "label_written":
            o[np.arange(R)[ok], lab[ok]] = 0
    q = quantise(o, fm, fmt, defect)
    cs = None
    if colsum0 is not None:
        cs = np.asarray(colsum0, F32).copy()
        for r0 in range(0, R, 256):
            blk = np.zeros((256, Vp), F32)
            blk[:min(256, R - r0)] = g[r0:r0 + 256]
            wsum = np.zeros((4, Vp), F32)
            for rg in range(4):
                for wv in range(4):
                    for rr in range(16):
                        wsum[wv] = (wsum[wv] + blk[rg * 64 + wv * 16 + rr]).astype(F32)
            s4 = ((wsum[0] + wsum[1]).astype(F32) + (wsum[2] + wsum[3]).astype(F32)).astype(F32)
            cs = (cs + (s4 * inv).astype(F32)).astype(F32)
    return dict(q=q, state=np.array([fm / inv, inv / fm], F32), coef=coef, colsum=cs)


# ------------------------------------------------------------------------------------------------ checks of the fused emitters
# Each takes the case's operands and `got`, a dict of numpy arrays read back from the device or produced by an emulation, so the GPU
# module and the check on the checker run the same assertions.
def check_emitted(src_written, amax_old, fmt, got, what):
    """bytes, state[1], the recorded amax and the table against emit_ref of the bf16 tensor as written"""
    b, sinv, amax = emit_ref(src_written, amax_old, fmt)
    check_bytes(got["q"], b, f"{what} bytes")
    check_state(got["state1"], np.asarray(got["table"], F32).max(), sinv, amax, what)
    check_table(got["table"], src_written, what)
    bad = ~is_finite_byte(got["q"], fmt)
    assert not bad.any(), f"{what}: a NaN / Inf byte"


def check_same_emission(got, kept, what):
    """the run that drops the bf16 copy: the kept run's bytes, state[1] and recorded amax"""
    assert np.array_equal(got["q"], kept["q"]), f"{what}: bytes differ from the run that keeps the bf16 tensor"
    assert F32(got["state1"]) == F32(kept["state1"]) and np.asarray(got["table"]).max() == np.asarray(kept["table"]).max(), what
    print(f"[conformance] {what}: {np.asarray(got['q']).size} bytes equal to the kept run's")


def check_ln_fwd_q8(x, gamma, beta, eps, p, seed, amax_old, fmt, got, what):
    """got: y [rows][W] (fp64 of the bf16 as written), mean, rstd, q, state1, table"""
    keep = RR.keep_mask(np.size(x), p, seed)
    f = RR.ln_fwd_ref(x, gamma, beta, eps, "bf16", keep, p)
    RR.check(got["mean"], f["mean"], f["bound_mean"], f"ln_fwd_q8/bf16 mean: {what}")
    RR.check(got["rstd"], f["rstd"], f["bound_rstd"], f"ln_fwd_q8/bf16 rstd: {what}")
    RR.check(got["y"], f["y"], f["bound_y"], f"ln_fwd_q8/bf16 y: {what}")
    check_emitted(got["y"], amax_old, fmt, got, f"ln_fwd_q8/{fmt}: {what}")
    return f


def check_ln_bwd_q8(x, gamma, mean, rstd, dy, dres, p, seed, mode, amax_old, fmt, got, what):
    """got: dx, dxm (None in mode 'dx'), part [2][nblk][W], q, state1, table; mean / rstd as handed to the kernel"""
    r = RR.ln_bwd_ref(x, gamma, mean, rstd, dy, "bf16", dres=dres)
    RR.check(got["dx"], r["dx"], r["bound_dx"], f"ln_bwd_q8/bf16 dx: {what}")
    src = got["dx"]
    if mode == "dxm":
        v, e = RR.dxm_ref(got["dx"], RR.keep_mask(np.size(x), p, seed), p, "bf16")
        RR.check(got["dxm"], v, e, f"ln_bwd_q8/bf16 dxm: {what}")
        src = got["dxm"]
    P = np.asarray(got["part"], np.float64)
    assert np.isfinite(P).all(), f"{what}: an entry of the partials was not written"
    RR.check(P[0].sum(0), r["dgamma"], r["bound_dgamma"], f"ln_bwd_q8/bf16 partials dgamma: {what}")
    RR.check(P[1].sum(0), r["dbeta"], r["bound_dbeta"], f"ln_bwd_q8/bf16 partials dbeta: {what}")
    check_emitted(src, amax_old, fmt, got, f"ln_bwd_q8/{fmt} {mode}: {what}")


def attn_problems(c, q_off):
    """(b, query rows, key rows) of every sequence"""
    B, Tq, Tk = c["B"], c["Tq"], c["Tk"]
    out = []
    for b in range(B):
        if c["q_len"] is None:
            out.append((b, slice(b * Tq, (b + 1) * Tq), slice(b * Tk, (b + 1) * Tk)))
        else:
            r = slice(int(q_off[b]), int(q_off[b]) + c["q_len"][b])
            out.append((b, r, r if c["kv_packed"] else slice(b * Tk, (b + 1) * Tk)))
    return out


def attn_q8_ref(c, q, k, v, do, km, q_off, out, lse):
    """fp64 dQ / dK / dV (util_attn_ref.bwd_ref on the out / lse the backward is handed, lse [B][H][Tq]) assembled as the byte tensors
    are laid out: [(name, y, bound, written rows)] — one [rows][3d] tensor for 'fused3', dQ [rows][d] and dK | dV [rows][2d] for 'kv2'"""
    import util_attn_ref as AR

    H, HD = c["H"], c["H"] * 64
    nq, nk = q.shape[0], k.shape[0]
    y = {n: np.zeros((r, HD)) for n, r in (("dQ", nq), ("dK", nk), ("dV", nk))}
    e = {n: np.zeros((r, HD)) for n, r in (("dQ", nq), ("dK", nk), ("dV", nk))}
    wq, wk = np.zeros(nq, bool), np.zeros(nk, bool)
    hd = lambda t: np.asarray(t).reshape(t.shape[0], H, 64).transpose(1, 0, 2)   # noqa: E731  [T][H*64] -> [H][T][64]
    for b, r, rk in attn_problems(c, q_off):
        n, m = r.stop - r.start, rk.stop - rk.start
        allowed = AR.allowed_mask(n, m, c["causal"], km[b][None, :] if km is not None else None)
        ref = AR.bwd_ref(hd(q[r]), hd(k[rk]), hd(v[rk]), hd(do[r]), allowed, "bf16", out=hd(out[r]), lse=lse[b, :, :n])
        for name, rows in (("dQ", r), ("dK", rk), ("dV", rk)):
            y[name][rows] = ref[name].transpose(1, 0, 2).reshape(-1, HD)
            e[name][rows] = ref["bound_" + name].transpose(1, 0, 2).reshape(-1, HD)
        wq[r], wk[rk] = True, True
    if c["layout"] == "fused3":
        return [("dQKV", np.concatenate([y["dQ"], y["dK"], y["dV"]], 1), np.concatenate([e["dQ"], e["dK"], e["dV"]], 1), wq)]
    return [("dQ", y["dQ"], e["dQ"], wq), ("dKV", np.concatenate([y["dK"], y["dV"]], 1), np.concatenate([e["dK"], e["dV"]], 1), wk)]


def attn_amax_old(refs, fmt="e5m2"):
    """half of the reference's maximum: the largest entries saturate"""
    return [float(F32(0.5 * np.abs(y[w]).max())) for _, y, _, w in refs]


def check_attn_q8(refs, amax_olds, fmt, got, what):
    """got: [(bytes [rows][cols], state1, table)] per tensor of refs.  -> the shares of bytes off the nominal one"""
    shares = []
    for (name, y, e, w), a_old, (b, st1, table) in zip(refs, amax_olds, got):
        lo, hi, nom = emit_interval(y[w], e[w], a_old, fmt)
        shares.append(check_interval(np.asarray(b)[w], lo, hi, nom, f"attn_bwd_q8/{fmt} {name}: {what}", fmt))
        assert F32(st1) == scale_of(a_old, fmt)[1], f"{what}: state[1] of {name}"
        t = np.asarray(table, F32)
        assert (t >= 0).all()
        check_amax_window(t.max(), y[w], e[w], f"attn_bwd_q8/{fmt} {name} amax: {what}")
    return shares


def check_ce_q8(x, V, labels, mask, ls, lse, denom, loss_scale, fmt, got, what, colsum0=None, plain=None):
    """got: q [rows][Vpad], state [2], coef [rows] | None, colsum [Vpad] | None.  plain: the bytes of the run without label_coef.
    Bounds beyond util_rowop_ref.ce_bwd_ref's e_g (per element of g = mask (softmax - soft)):
      state    inv = fl32(loss_scale / denom), state[1] = fl32(inv / FMAX), state[0] = fl32(FMAX / inv): two roundings, 3 u32 relative
      coef     g_label inv: e_g inv + 3 u32 |coef| (inv's rounding, the product's, and g's own are in e_g)
      colsum   start + inv sum_rows g: inv sum e_g  +  gamma_(rows + 2) inv sum |g| (one fp32 rounding per addend of the column's sum
               in any order, the product with inv, inv itself)  +  A u32 (|start| + inv sum |g|) for the A = ceil(rows / 256) atomic
               adds, each rounding a partial result no larger than that
    -> the share of bytes off the nominal one"""
    from util_gemm_ref import U32, gamma_k

    x = np.asarray(x, np.float64)
    R, Vp = x.shape
    g, e = ce_q8_ref(np.nan_to_num(x), V, labels, mask, ls, lse)
    lab = np.asarray(labels)
    ok = (lab >= 0) & (lab < V)
    ar = np.arange(R)
    q = np.asarray(got["q"], np.uint8)
    assert not q[:, V:].any(), f"{what}: padding columns V .. Vpad are not zero bytes"
    assert not (q[np.asarray(mask) == 0] & 0x7F).any(), f"{what}: a masked row is not all zero bytes"
    gq, eq = g.copy(), e.copy()
    if got.get("coef") is not None:
        assert not (q[ar[ok], lab[ok]] & 0x7F).any(), f"{what}: a label byte was written in label_coef mode"
        gq[ar[ok], lab[ok]], eq[ar[ok], lab[ok]] = 0.0, 0.0
        if plain is not None:
            p1 = np.array(plain, np.uint8)
            p1[ar[ok], lab[ok]] = 0
            check_bytes(q, p1, f"ce_bwd_q8/{fmt} label_coef bytes = plain bytes without the labels: {what}")
    lo, hi, nom = emit_interval(gq, eq, 1.0, fmt, store="f32")   # amax_old 1: scale = FMAX, the closed form
    share = check_interval(q, lo, hi, nom, f"ce_bwd_q8/{fmt} dlogits ls={ls}: {what}", fmt)
    inv = float(F32(loss_scale)) / float(denom)
    s0, s1 = FMAX[fmt] / inv, inv / FMAX[fmt]
    RR.check(np.asarray(got["state"], np.float64), [s0, s1], [3 * U32 * s0, 3 * U32 * s1], f"ce_bwd_q8/{fmt} state: {what}")
    if got.get("coef") is not None:
        cref = np.where(ok, g[ar, np.where(ok, lab, 0)] * inv, 0.0)
        cb = np.where(ok, e[ar, np.where(ok, lab, 0)] * inv + 3 * U32 * np.abs(cref), 0.0) + 1e-300
        RR.check(got["coef"], cref, cb, f"ce_bwd_q8/{fmt} label_coef ls={ls}: {what}")
        assert not np.asarray(got["coef"])[~ok].any(), f"{what}: the coefficient of a label outside [0, V) is not cleared"
    if got.get("colsum") is not None:
        A = -(-R // 256)
        a = inv * np.abs(g).sum(0)
        ref = colsum0 + inv * g.sum(0)
        bound = inv * e.sum(0) + gamma_k(R + 2) * a + A * U32 * (np.abs(colsum0) + a) + 1e-300
        RR.check(got["colsum"], ref, bound, f"ce_bwd_q8/{fmt} colsum ls={ls}: {what}")
        assert np.array_equal(np.asarray(got["colsum"], F32)[V:], np.asarray(colsum0, F32)[V:]), f"{what}: colsum of a padding column moved"
    return share
