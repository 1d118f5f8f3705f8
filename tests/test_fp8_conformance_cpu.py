"""CPU checks of the fp8 emission conformance suite itself (tests/test_fp8_conformance_gpu.py needs the MI355X):
  - the encoder of tests/util_fp8_ref.py, built from the OCP value tables alone, agrees with torch's cast and with a brute-force
    nearest-value search on every finite bf16 value times a table of scales;
  - numpy emulations of every emitter's arithmetic pass the checks the GPU module applies, on the same case operands;
  - seeded defects, each an emulation with one flaw, are rejected by those checks; for the interval-checked emitters (attention
    backward, CE backward) this also shows that the intervals are not vacuous (INTERVAL_DEFECTS lists what each case rejects);
  - the set of kernels in scope is computed from tests/golden/kernel_resources.json by name pattern — the ten fp8-emitting instantiations
    outside the GEMM epilogues — and every one appears in the committed kernel listing of the GPU module."""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_attn_ref as AR  # noqa: E402
import util_fp8_cases as FC  # noqa: E402
import util_fp8_ref as FR  # noqa: E402
import util_rowop_cases as RC  # noqa: E402
import util_rowop_ref as RR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COVERAGE_PROFILE = "profiles/fp8_conformance_kernel_stats.txt"
TFMT = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
SCALES = (2.0 ** -100, 2.0 ** -20, 1.0 / 3.0, 1.0, 448.0 / 3.1416, 2.0 ** 40, 3.0e38)
F32 = np.float32


def rejected(fn, label):
    """the check raises; what it printed on the way (the defective run's own [conformance] lines) is dropped"""
    with pytest.raises(AssertionError), contextlib.redirect_stdout(io.StringIO()):
        fn()
    print(f"[rejected] {label}")


# ------------------------------------------------------------------------------------------------ the encoder
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_q8_encode_on_every_finite_bf16(fmt):
    v = FC.all_finite_bf16().reshape(-1)
    fm = F32(FR.FMAX[fmt])
    for sc in SCALES:
        with np.errstate(over="ignore"):
            t = np.clip((v * F32(sc)).astype(F32), -fm, fm)
        got = FR.q8_encode(t, fmt)
        assert np.array_equal(got, torch.from_numpy(t).to(TFMT[fmt]).view(torch.uint8).numpy()), f"{fmt} scale {sc}: differs from torch's cast"
        assert np.array_equal(got, FR.q8_brute(t, fmt)), f"{fmt} scale {sc}: differs from the nearest-value search"
        assert FR.is_finite_byte(got, fmt).all()
    # saturation and the sign of zero
    big = np.array([1e30, -1e30, np.inf, -np.inf, 0.0, -0.0, 1e-30, -1e-30], F32)
    top = len(FR.GRID[fmt]) - 1
    assert FR.q8_encode(big, fmt).tolist() == [top, top | 0x80, top, top | 0x80, 0, 0x80, 0, 0x80]


def test_rounding_boundaries_are_ties_to_even():
    """the midpoint of two neighbouring values goes to the even byte, one fp32 step to either side to the nearer one"""
    for fmt in FR.FMTS:
        g = FR.GRID[fmt]
        mid = ((g[:-1] + g[1:]) / 2).astype(F32)
        assert np.array_equal(mid.astype(np.float64), (g[:-1] + g[1:]) / 2)
        b = np.arange(len(g) - 1)
        assert np.array_equal(FR.q8_encode(mid, fmt), np.where(b % 2 == 0, b, b + 1))
        assert np.array_equal(FR.q8_encode(np.nextafter(mid, F32(0)), fmt), b)
        assert np.array_equal(FR.q8_encode(np.nextafter(mid, F32(np.inf)), fmt), b + 1)


def test_interval_ends():
    x = np.array([1.0000001, -1.0000001, 0.0, 1.0, 3.0e-41, -3.3e38])
    d, u = FR.bf16_down(x), FR.bf16_up(x)
    assert (d <= x).all() and (u >= x).all() and np.array_equal(FR.round_bf16(d), d) and np.array_equal(FR.round_bf16(u), u)
    assert d[0] == 1.0 and u[0] == 1.0078125 and d[2] == u[2] == 0.0 and d[3] == u[3] == 1.0
    assert (FR._bf16_key(u) - FR._bf16_key(d) <= 1).all()


# ------------------------------------------------------------------------------------------------ quantiser
QUANT_DEFECTS = ["fnuz", "truncate", "flush_subnormals", "no_clamp", "scale_inverted", "state1_new"]


def _exh(kind, fmt):
    a = FC.EXH_AMAX[kind]
    return FC.tiny_amax(fmt) if a == "tiny" else a


@pytest.mark.parametrize("kind", list(FC.EXH_AMAX))
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_quantiser_emulation_every_finite_bf16(fmt, kind):
    v, a_old = FC.all_finite_bf16(), _exh(kind, fmt)
    FR.check_quant(FR.quant_expect(v, 256, 256, 256, fmt, a_old), FR.emu_quantize(v, 256, 256, 256, fmt, a_old), f"every finite bf16, {kind}", fmt)


@pytest.mark.parametrize("defect", QUANT_DEFECTS)
@pytest.mark.parametrize("fmt", FR.FMTS)
def test_quantiser_defects_rejected_on_every_finite_bf16(fmt, defect):
    """delayed scaling at the non-power-of-two amax ('no_fabs' is seeded in the geometry cases, whose largest magnitude is negative)"""
    v = FC.all_finite_bf16()
    a_old = FC.EXH_AMAX["nonpow2"]
    exp = FR.quant_expect(v, 256, 256, 256, fmt, a_old)
    rejected(lambda: FR.check_quant(exp, FR.emu_quantize(v, 256, 256, 256, fmt, a_old, defect), defect, fmt), f"quantiser/{fmt}: {defect}")


@pytest.mark.parametrize("fmt", FR.FMTS)
def test_infinite_scale_is_rejected(fmt):
    """the defect the tiny-amax cases are there for: FMAX / amax_old = inf, 0 * inf = NaN, clamped to -FMAX"""
    v, a_old = FC.all_finite_bf16(), FC.tiny_amax(fmt)
    bad = FR.emu_quantize(v, 256, 256, 256, fmt, a_old, "inf_scale")
    fm = F32(FR.FMAX[fmt])
    with np.errstate(invalid="ignore", over="ignore"):
        t = (v * F32(np.inf)).astype(F32)
        t = np.where(np.isnan(t), -fm, np.clip(t, -fm, fm))   # IEEE minNum / maxNum: the NaN operand is dropped, fmaxf(NaN, -fm) = -fm
    bad["q"] = FR.q8_encode(t, fmt)
    assert (bad["q"][v == 0] == (len(FR.GRID[fmt]) - 1) | 0x80).all()
    rejected(lambda: FR.check_quant(FR.quant_expect(v, 256, 256, 256, fmt, a_old), bad, "inf_scale", fmt), f"quantiser/{fmt}: infinite scale")


@pytest.mark.parametrize("fmt", FR.FMTS)
@pytest.mark.parametrize("name", [g[0] for g in FC.GEOMETRY])
def test_quantiser_emulation_geometry(name, fmt):
    _, rows, cols, rp, _, _, _ = FC.GEOMETRY_BY[name]
    full = FC.geometry_source(name, fmt)
    for a_old in (None, 4.0):
        exp = FR.quant_expect(full, rows, cols, rp, fmt, a_old)
        FR.check_quant(exp, FR.emu_quantize(full, rows, cols, rp, fmt, a_old), name, fmt)
        for defect in ("amax_over_padding", "qT_pad_canary", "no_fabs"):
            if defect == "qT_pad_canary" and rp == rows:
                continue
            rejected(lambda: FR.check_quant(exp, FR.emu_quantize(full, rows, cols, rp, fmt, a_old, defect), defect, fmt),
                     f"quantiser/{fmt} {name} {'current' if a_old is None else 'delayed'}: {defect}")


def test_partial_table_wrap_and_roll():
    rows, cols = FC.WRAP["rows"], FC.WRAP["cols"]
    v = FC.wrap_source()
    exp = FR.quant_expect(v, rows, cols, rows, "e4m3", 6.0)
    FR.check_quant(exp, FR.emu_quantize(v, rows, cols, rows, "e4m3", 6.0), "131200x64", "e4m3")
    rejected(lambda: FR.check_quant(exp, FR.emu_quantize(v, rows, cols, rows, "e4m3", 6.0, "no_wrap"), "no_wrap", "e4m3"),
             "quantiser: partial index not wrapped, the write dropped")
    s0, p0 = FC.roll_inputs()
    FR.check_roll(s0, p0, *FR.emu_roll(s0, p0), "5 slots, stride 3")
    rejected(lambda: FR.check_roll(s0, p0, *FR.emu_roll(s0, p0, "no_clear"), "no_clear"), "roll: table not cleared")


# ------------------------------------------------------------------------------------------------ LayerNorm
def _ln_fwd_emu(x, g, b, p, a_old, fmt, defect=None):
    keep = RR.keep_mask(x.size, p, FC.LN_SEED)
    y32, mean, rstd = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, "f32", keep, p)    # the fp32 results before the store
    q, st1, amax = FR.emu_emit(y32, a_old, fmt, defect)
    table = np.zeros(FR.PARTIALS, F32)
    rowmax = np.abs(FR.round_bf16(y32.astype(np.float64))).max(1).astype(F32)
    idx = np.arange(x.shape[0])
    ok = idx < FR.PARTIALS if defect == "no_wrap" else np.ones(len(idx), bool)
    np.maximum.at(table, idx[ok] & (FR.PARTIALS - 1), rowmax[ok])
    if defect == "no_fabs":
        table = np.minimum(table, amax).astype(F32)
    return dict(y=FR.round_bf16(y32.astype(np.float64)), mean=mean, rstd=rstd, q=q, state1=st1, table=table)


@pytest.mark.parametrize("p", FC.LN_DROPOUT)
@pytest.mark.parametrize("rows,width", FC.LN_SHAPES)
def test_ln_fwd_q8_emulation_and_defects(rows, width, p):
    x, g, b, _, _ = RC.ln_inputs(FC.ln_case(rows, width), "bf16")
    keep = RR.keep_mask(x.size, p, FC.LN_SEED)
    a_old = float(F32(0.6 * np.abs(RR.ln_fwd_ref(x, g, b, RC.LN_EPS, "bf16", keep, p)["y"]).max()))
    what = f"{rows}x{width} p={p}"
    FR.check_ln_fwd_q8(x, g, b, RC.LN_EPS, p, FC.LN_SEED, a_old, "e4m3", _ln_fwd_emu(x, g, b, p, a_old, "e4m3"), what)
    for defect in ("fnuz", "truncate", "no_clamp", "scale_inverted", "state1_new") + (("no_bf16_rounding",) if width >= 72 else ()):
        rejected(lambda: FR.check_ln_fwd_q8(x, g, b, RC.LN_EPS, p, FC.LN_SEED, a_old, "e4m3", _ln_fwd_emu(x, g, b, p, a_old, "e4m3", defect), what),
                 f"ln_fwd_q8 {what}: {defect}")


def test_ln_fwd_q8_wave_index_wrap():
    x, g, b = FC.ln_wrap_inputs()
    FR.check_ln_fwd_q8(x, g, b, RC.LN_EPS, 0.0, FC.LN_SEED, 1.0, "e5m2", _ln_fwd_emu(x, g, b, 0.0, 1.0, "e5m2"), "1030x8")
    rejected(lambda: FR.check_ln_fwd_q8(x, g, b, RC.LN_EPS, 0.0, FC.LN_SEED, 1.0, "e5m2", _ln_fwd_emu(x, g, b, 0.0, 1.0, "e5m2", "no_wrap"), "1030x8"),
             "ln_fwd_q8: wave index not wrapped, the write dropped")


def _ln_bwd_emu(x, g, mean, rstd, dy, dres, p, mode, a_old, fmt, defect=None):
    dx, _, _, part = RR.emu_ln_bwd(x, g, mean, rstd, dy, "bf16", dres=dres)
    src32 = dx
    dxm = None
    if mode == "dxm":
        keep = RR.keep_mask(x.size, p, 9).reshape(x.shape)
        sc = (F32(1) / (F32(1) - F32(p))) if p > 0 else F32(1)
        src32 = np.where(keep, (dx * sc).astype(F32), F32(0))
        dxm = FR.round_bf16(src32.astype(np.float64))
    q, st1, amax = FR.emu_emit(src32, a_old, fmt, defect)
    table = np.zeros(FR.PARTIALS, F32)
    table[0] = amax
    return dict(dx=dx.astype(np.float64), dxm=dxm, part=part, q=q, state1=st1, table=table)


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("mode,p", FC.LNB_MODES)
@pytest.mark.parametrize("rows,width", FC.LNB_SHAPES)
def test_ln_bwd_q8_emulation_and_defects(rows, width, mode, p, with_dres):
    x, g, b, dy, dres = RC.ln_inputs(FC.ln_case(rows, width), "bf16")
    mean, rstd = RR.emu_ln_fwd(x, g, b, RC.LN_EPS, "bf16")[1:]
    dr = dres if with_dres else None
    a_old = float(F32(0.6 * np.abs(RR.ln_bwd_ref(x, g, mean, rstd, dy, "bf16", dres=dr)["dx"]).max()))
    what = f"{rows}x{width} {mode} p={p}"
    FR.check_ln_bwd_q8(x, g, mean, rstd, dy, dr, p, 9, mode, a_old, "e5m2", _ln_bwd_emu(x, g, mean, rstd, dy, dr, p, mode, a_old, "e5m2"), what)
    for defect in ("fnuz", "truncate", "no_clamp", "scale_inverted", "state1_new") + (("no_bf16_rounding",) if mode == "dxm" and p > 0 else ()):
        rejected(lambda: FR.check_ln_bwd_q8(x, g, mean, rstd, dy, dr, p, 9, mode, a_old, "e5m2",
                                            _ln_bwd_emu(x, g, mean, rstd, dy, dr, p, mode, a_old, "e5m2", defect), what), f"ln_bwd_q8 {what}: {defect}")


# ------------------------------------------------------------------------------------------------ interval-checked emitters
# what each case of the interval-checked emitters rejects (every entry is asserted below)
INTERVAL_DEFECTS = {
    # every attention case; subnormals flushed and the missing bf16 rounding on aq_vit_50x50 (the first under a scale that puts the
    # gradients on subnormal bytes, the second through the recorded amax, which is then no bf16 value: the byte intervals admit it)
    "attn": ("fnuz", "truncate", "no_clamp", "scale_inverted", "state[1] of another amax", "amax 10 % low", "flush_subnormals", "no_bf16_rounding"),
    # every CE case; subnormals flushed in e4m3 only (g FMAX reaches the e5m2 subnormals, below 6.1e-5, for no element of these cases)
    "ce": ("fnuz", "truncate", "flush_subnormals", "label_written", "pad_cols"),
}


def _attn_emu(c, a_olds=None, fmt="e5m2", defect=None):
    """forward and backward emulations per problem (bf16 storage), the stored gradients assembled and emitted"""
    q, k, v, do, km, q_off = FC.attn_inputs(c)
    B, H, Tq, HD = c["B"], c["H"], c["Tq"], c["H"] * 64
    out, lse = np.zeros((q.shape[0], HD)), np.zeros((B, H, Tq))
    g32 = {n: np.zeros((r, HD), F32) for n, r in (("dQ", q.shape[0]), ("dK", k.shape[0]), ("dV", k.shape[0]))}
    for b, r, rk in FR.attn_problems(c, q_off):
        n, m = r.stop - r.start, rk.stop - rk.start
        allowed = AR.allowed_mask(n, m, c["causal"], km[b] if km is not None else None)
        for h in range(H):
            cs = slice(h * 64, (h + 1) * 64)
            o, l = AR.emu_fwd(q[r, cs], k[rk, cs], v[rk, cs], allowed, "bf16")
            out[r, cs], lse[b, h, :n] = o, l
            dq, dk, dv = AR.emu_bwd(q[r, cs], k[rk, cs], v[rk, cs], o, do[r, cs], l, allowed, "f32" if defect == "no_bf16_rounding" else "bf16")
            g32["dQ"][r, cs], g32["dK"][rk, cs], g32["dV"][rk, cs] = dq, dk, dv
    refs = FR.attn_q8_ref(c, q, k, v, do, km, q_off, out, lse)
    a_olds = FR.attn_amax_old(refs) if a_olds is None else a_olds
    tens = [np.concatenate([g32["dQ"], g32["dK"], g32["dV"]], 1)] if c["layout"] == "fused3" else [g32["dQ"], np.concatenate([g32["dK"], g32["dV"]], 1)]
    got = []
    for t, a, (_, _, _, w) in zip(tens, a_olds, refs):
        qb, st1, amax = FR.emu_emit(t, a, fmt, defect, valid=w)
        table = np.zeros(FR.PARTIALS, F32)
        table[3] = amax
        got.append((qb, st1, table))
    return refs, a_olds, got


@pytest.mark.parametrize("name", [c["name"] for c in FC.ATTN])
def test_attn_bwd_q8_emulation_and_defects(name):
    c = FC.ATTN_BY[name]
    refs, a_olds, got = _attn_emu(c)
    shares = FR.check_attn_q8(refs, a_olds, "e5m2", got, name)
    print(f"[share] attn_bwd_q8 emulation {name}: {max(shares):.3g}")
    for defect in ("fnuz", "truncate", "no_clamp", "scale_inverted"):
        rejected(lambda: FR.check_attn_q8(refs, a_olds, "e5m2", _attn_emu(c, a_olds, defect=defect)[2], name), f"attn_bwd_q8 {name}: {defect}")
    wrong = [(b, st1 * F32(2), t) for b, st1, t in got]
    rejected(lambda: FR.check_attn_q8(refs, a_olds, "e5m2", wrong, name), f"attn_bwd_q8 {name}: state[1] from another amax")
    low = [(b, st1, t * F32(0.9)) for b, st1, t in got]
    rejected(lambda: FR.check_attn_q8(refs, a_olds, "e5m2", low, name), f"attn_bwd_q8 {name}: recorded amax 10 % low")


def test_attn_bwd_q8_subnormal_flush_and_fp32_source():
    """under a scale that puts the gradients on subnormal bytes a flush is rejected; quantising the fp32 accumulators without the bf16
    rounding stays inside the byte intervals (they admit every bf16 value within the bound) and is rejected by the recorded amax,
    which is then no bf16 value"""
    c = FC.ATTN_BY["aq_vit_50x50"]
    refs, _, _ = _attn_emu(c)
    big = [float(F32(2.0 ** 31 * np.abs(refs[0][1]).max()))]
    FR.check_attn_q8(refs, big, "e5m2", _attn_emu(c, big)[2], "subnormal outputs")
    rejected(lambda: FR.check_attn_q8(refs, big, "e5m2", _attn_emu(c, big, defect="flush_subnormals")[2], "flush"), "attn_bwd_q8: subnormals flushed")
    r2, a2, g2 = _attn_emu(c, defect="no_bf16_rounding")
    rejected(lambda: FR.check_attn_q8(r2, a2, "e5m2", g2, "no bf16 rounding"), "attn_bwd_q8: fp32 quantised without the bf16 rounding")


@pytest.mark.parametrize("V,Vpad", FC.CE_V)
@pytest.mark.parametrize("rows", FC.CE_ROWS)
def test_ce_bwd_q8_emulation_and_defects(rows, V, Vpad):
    x, labels, mask, lse, denom = FC.ce_inputs(rows, V, Vpad)
    xs = np.nan_to_num(x, nan=7.0)   # what the padding columns hold is discarded
    start = np.linspace(-1, 1, Vpad).astype(F32).astype(np.float64) * 1e-3
    for fmt in FR.FMTS:
        for ls in FC.CE_LS:
            what = f"{rows}x{V}/{Vpad} {fmt} ls={ls}"
            plain = FR.emu_ce_bwd_q8(xs, V, labels, mask, ls, lse, denom, FC.CE_LOSS_SCALE, fmt, colsum0=start)
            FR.check_ce_q8(x, V, labels, mask, ls, lse, denom, FC.CE_LOSS_SCALE, fmt, plain, what, colsum0=start)
            coef = FR.emu_ce_bwd_q8(xs, V, labels, mask, ls, lse, denom, FC.CE_LOSS_SCALE, fmt, label_coef=True, colsum0=start)
            FR.check_ce_q8(x, V, labels, mask, ls, lse, denom, FC.CE_LOSS_SCALE, fmt, coef, what + " label_coef", colsum0=start, plain=plain["q"])
            for defect in ("fnuz", "truncate", "label_written", "pad_cols") + (("flush_subnormals",) if fmt == "e4m3" else ()):
                bad = FR.emu_ce_bwd_q8(xs, V, labels, mask, ls, lse, denom, FC.CE_LOSS_SCALE, fmt, label_coef=defect == "label_written",
                                       colsum0=start, defect=defect)
                rejected(lambda: FR.check_ce_q8(x, V, labels, mask, ls, lse, denom, FC.CE_LOSS_SCALE, fmt, bad, what, colsum0=start), f"ce_bwd_q8 {what}: {defect}")


# ------------------------------------------------------------------------------------------------ coverage
def _instantiations(path):
    pat = r"\b(?:fp8_[a-z]+_kernel|ln_[a-z_]*kernel|attn_bwd_kernel|ce_bwd_q8_kernel)(?:<[^>]*>)?"
    with open(os.path.join(ROOT, path)) as f:
        return {re.sub(r"\s+", "", m) for m in re.findall(pat, f.read())}


def test_every_instantiation_in_scope_is_launched():
    ns = lambda names: {re.sub(r"\s+", "", n) for n in names}  # noqa: E731
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")))
    built = {k for unit in table.values() for k in unit if re.match(FC.IN_SCOPE, k)}
    assert len(built) == 10 and ns(built) == ns(FC.KERNELS), sorted(ns(built) ^ ns(FC.KERNELS))
    traced = _instantiations(COVERAGE_PROFILE)
    assert ns(FC.KERNELS) <= traced, sorted(ns(FC.KERNELS) - traced)
    gpu = open(os.path.join(ROOT, "tests", "test_fp8_conformance_gpu.py")).read()
    for k in ("fp8_amax_kernel", "fp8_quantize_kernel", "fp8_roll_kernel", "ln_fwd_kernel<unsigned short, true>", "ln_bwd_kernel<unsigned short, {2,4}, 8, {1,2}>",
              "attn_bwd_kernel<unsigned short, true>", "ce_bwd_q8_kernel"):
        assert k in gpu, f"the GPU module's docstring does not list {k}"
    assert {FC.lnb_kernel(w, m) for _, w in FC.LNB_SHAPES for m, _ in FC.LNB_MODES} == {k for k in FC.KERNELS if k.startswith("ln_bwd")}
