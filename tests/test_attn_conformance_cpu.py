"""The attention conformance suite's own checks, on a machine without a GPU:
  - numpy emulations of the kernels' arithmetic (tests/util_attn_ref.py: bf16 single-tile forward / backward, the online-softmax
    walk over 64-key blocks, the fp32 path, decode with the running (max, sum, out) triple) are accepted by the fp64 reference's
    bounds at the table's shapes;
  - seeded defects are rejected — among them the ones the max-scaled tolerance of tests/test_ops_gpu.py accepts;
  - the canaries see a store one row past a packed sequence and an lse entry past q_len[b];
  - every case of tests/util_attn_cases.py reaches the kernel it claims (a pure mirror of the dispatch rules of csrc/attention.hip),
    and the committed kernel trace of the GPU module holds every claimed instantiation, every attention kernel of the build and of
    the product's committed profiles."""
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import util_attn_cases as AC  # noqa: E402
import util_attn_ref as AR  # noqa: E402
import util_gemm_ref as GR  # noqa: E402

PRODUCT_PROFILES = ("profiles/r6_train_kernel_stats_serial.txt", "profiles/r6_train_fp8_kernel_stats_serial.txt",
                    "profiles/r6_generate_kernel_stats.txt")
COVERAGE_PROFILE = "profiles/attn_conformance_kernel_stats.txt"
Q8_KERNEL = "attn_bwd_kernel<unsigned short, true>"  # fp8 emission: tests/test_fp8_conformance_gpu.py
OLD_TOL, OLD_TOL_GRAD = 1.2e-2, 3e-2


def problem(Tq, Tk, dtype, seed=0, qscale=1.0):
    rng = np.random.default_rng(seed)
    q, k, v, do = (GR.round_to(rng.standard_normal((n, 64)), dtype) for n in (Tq, Tk, Tk, Tq))
    return GR.round_to(q * qscale, dtype), k, v, do


def _rejects(fn, *a):
    with pytest.raises(AssertionError):
        fn(*a)


def _accept_fwd(q, k, v, allowed, dtype, block, what):
    out, lse = AR.emu_fwd(q, k, v, allowed, dtype, block=block)
    f = AR.fwd_ref(q, k, v, allowed, dtype)
    w = [AR.check(out, f["O"], f["bound_O"], what + " out"), AR.check_lse(lse, f["lse"], f["bound_lse"], what + " lse")]
    return out, lse, max(w)


def _accept_bwd(q, k, v, do, out, lse, allowed, dtype, block, what):
    got = AR.emu_bwd(q, k, v, out, do, lse, allowed, dtype, block=block)
    b = AR.bwd_ref(q, k, v, do, allowed, dtype, out=out, lse=lse)
    e = AR.bwd_ref(q, k, v, do, allowed, dtype)
    for g, n in zip(got, ("dQ", "dK", "dV")):
        AR.check(g, b[n], b["bound_" + n], f"{what} {n}")
        AR.check(g, e[n], e["bound_" + n], f"{what} {n} end to end")
    return got, b


SHAPES = [(64, 64, True, 1.0), (50, 50, False, 1.0), (64, 50, False, 1.0), (33, 64, False, 1.0), (64, 64, True, 4.0), (1, 1, False, 1.0),
          (31, 64, True, 1.0), (64, 32, True, 1.0)]
TILED_SHAPES = [(65, 65, True, 1.0), (128, 128, True, 1.0), (197, 197, False, 1.0), (50, 197, True, 1.0), (130, 50, True, 1.0),
                (129, 197, False, 4.0), (65, 200, False, 8.0)]


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("Tq,Tk,causal,qscale", SHAPES)
def test_bounds_accept_the_single_tile_arithmetic(dtype, Tq, Tk, causal, qscale):
    q, k, v, do = problem(Tq, Tk, dtype, Tq * 100 + Tk, qscale)
    allowed = AR.allowed_mask(Tq, Tk, causal)
    out, lse, _ = _accept_fwd(q, k, v, allowed, dtype, None, f"single {Tq}x{Tk} {dtype}")
    _accept_bwd(q, k, v, do, out, lse, allowed, dtype, None, f"single {Tq}x{Tk} {dtype}")


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("Tq,Tk,causal,qscale", TILED_SHAPES)
def test_bounds_accept_the_online_softmax_walk(dtype, Tq, Tk, causal, qscale):
    q, k, v, do = problem(Tq, Tk, dtype, Tq * 100 + Tk, qscale)
    k[Tk - 2] *= 3.0  # a dominant key in the last block: the running maximum moves late
    km = np.ones(Tk, np.int32)
    km[Tk // 2] = 0
    allowed = AR.allowed_mask(Tq, Tk, causal, km)
    out, lse, _ = _accept_fwd(q, k, v, allowed, dtype, 64, f"tiled {Tq}x{Tk} {dtype}")
    _accept_bwd(q, k, v, do, out, lse, allowed, dtype, 64, f"tiled {Tq}x{Tk} {dtype}")


@pytest.mark.parametrize("dtype", AC.DTYPES)
def test_bounds_accept_a_shifted_row_and_a_row_without_keys(dtype):
    """a constant of 20 on every score (shift invariance), a first block entirely masked, and rows with no admissible key: zeros,
    lse = -inf, and finite gradients everywhere"""
    Tq, Tk = 70, 130
    q, k, v, do = problem(Tq, Tk, dtype, 5)
    q[:, 0], k[:, 0] = 16.0, 10.0
    km = np.ones(Tk, np.int32)
    km[:64] = 0
    allowed = AR.allowed_mask(Tq, Tk, False, km)
    allowed[3] = False
    allowed[69] = False
    out, lse, _ = _accept_fwd(q, k, v, allowed, dtype, 64, f"shifted {dtype}")
    assert np.isneginf(lse[[3, 69]]).all() and not out[[3, 69]].any() and np.isfinite(lse[:3]).all()
    got, b = _accept_bwd(q, k, v, do, out, lse, allowed, dtype, 64, f"shifted {dtype}")
    assert all(np.isfinite(g).all() for g in got) and not got[0][[3, 69]].any() and not b["dQ"][[3, 69]].any()


def _decode_problem(dtype, R, H, L, seed):
    rng = np.random.default_rng(seed)
    kc, vc = (GR.round_to(rng.standard_normal((R, L, H * 64)), dtype) for _ in range(2))
    kc[2, L - 3] *= 6.0
    q = GR.round_to(rng.standard_normal((R, H * 64)), dtype)
    src = rng.integers(0, R, (R, L)).astype(np.int32)
    return q, kc, vc, src


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("L,cur", [(64, 0), (64, 63), (200, 64), (200, 199), (130, 140)])
def test_bounds_accept_the_decode_arithmetic(dtype, L, cur):
    R, H = 5, 2
    q, kc, vc, src = _decode_problem(dtype, R, H, L, L + cur)
    for kw in (dict(src_row=src), dict(row_div=4)):
        ref, bound = AR.decode_ref(q, kc, vc, H, L, cur, dtype, **kw)
        AR.check(AR.emu_decode(q, kc, vc, H, L, cur, dtype, **kw), ref, bound, f"decode {L}/{cur} {dtype} {list(kw)[0]}")


# ---------------------------------------------------------------------------------------------------------- seeded defects
def test_rejects_a_padded_key_in_the_row_sum_which_the_old_tolerance_accepts():
    """the tile is zero padded to 64 keys: one padded row counted in the row sum (score q.0 = 0) scales every output row by
    l / (l + exp(-max)).  Caught on `out` and `lse` at 50x50 (where max |err| / max |ref| is 1.1e-2 .. 1.3e-2 by seed: at the edge
    of the old 1.2e-2) and on `lse` at 197x197, where the old criterion accepts `out` outright — and `lse` was compared with
    nothing."""
    q, k, v, _ = problem(50, 50, "bf16", 0)
    allowed = AR.allowed_mask(50, 50)
    f = AR.fwd_ref(q, k, v, allowed, "bf16")
    out, lse = AR.emu_fwd(q, k, v, allowed, "bf16", defect="pad_key_in_sum")
    _rejects(AR.check, out, f["O"], f["bound_O"], "50x50 out, padded key in the row sum")
    _rejects(AR.check_lse, lse, f["lse"], f["bound_lse"], "50x50 lse, padded key in the row sum")
    q, k, v, _ = problem(197, 197, "bf16", 1)
    allowed = AR.allowed_mask(197, 197)
    f = AR.fwd_ref(q, k, v, allowed, "bf16")
    out, lse = AR.emu_fwd(q, k, v, allowed, "bf16", block=64, defect="pad_key_in_sum")
    _rejects(AR.check_lse, lse, f["lse"], f["bound_lse"], "197x197 lse, padded key in the row sum")
    assert AR.old_criterion(out, f["O"]) < OLD_TOL


def test_rejects_an_ignored_key_mask_bit_which_the_old_tolerance_accepts():
    """one masked key of the last block attended anyway (finite values of ordinary size behind the mask).  Masks are per batch
    entry, and the old criterion divides by the largest element of the WHOLE tensor: with a second, unmasked entry whose values are
    32 times larger (heads and layers do differ that much), the damaged entry's error of 15 % of its own scale disappears."""
    Tq, Tk = 197, 197
    q, k, v, do = problem(Tq, Tk, "bf16", 2)
    v, do = v / 32, do / 32
    km = np.ones(Tk, np.int32)
    km[Tk - 3:] = 0
    allowed = AR.allowed_mask(Tq, Tk, False, km)
    leaky = allowed.copy()
    leaky[:, Tk - 2] = True
    q0, k0, v0, do0 = problem(Tq, Tk, "bf16", 20)  # the other batch entry: no mask, nothing wrong
    full = AR.allowed_mask(Tq, Tk)
    f0 = AR.fwd_ref(q0, k0, v0, full, "bf16")
    out0, lse0 = AR.emu_fwd(q0, k0, v0, full, "bf16", block=64)
    f = AR.fwd_ref(q, k, v, allowed, "bf16")
    out, lse = AR.emu_fwd(q, k, v, leaky, "bf16", block=64)
    _rejects(AR.check, out, f["O"], f["bound_O"], "out, mask bit ignored")
    _rejects(AR.check_lse, lse, f["lse"], f["bound_lse"], "lse, mask bit ignored")
    assert AR.old_criterion(out, f["O"]) > 5 * OLD_TOL  # alone it would have been seen ...
    assert AR.old_criterion(np.stack([out0, out]), np.stack([f0["O"], f["O"]])) < OLD_TOL  # ... in the batch it is not
    # the backward with the same leak, on a correct forward's out / lse: dV of the masked key is not zero
    out, lse = AR.emu_fwd(q, k, v, allowed, "bf16", block=64)
    b = AR.bwd_ref(q, k, v, do, allowed, "bf16", out=out, lse=lse)
    got = AR.emu_bwd(q, k, v, out, do, lse, leaky, "bf16", block=64)
    b0 = AR.bwd_ref(q0, k0, v0, do0, full, "bf16", out=out0, lse=lse0)
    got0 = AR.emu_bwd(q0, k0, v0, out0, do0, lse0, full, "bf16", block=64)
    for i, n in enumerate(("dQ", "dK", "dV")):
        _rejects(AR.check, got[i], b[n], b["bound_" + n], n + ", mask bit ignored")
        assert AR.old_criterion(np.stack([got0[i], got[i]]), np.stack([b0[n], b[n]])) < OLD_TOL_GRAD


@pytest.mark.parametrize("dtype", AC.DTYPES)
def test_rejects_causal_off_by_one(dtype):
    Tq = Tk = 64
    q, k, v, do = problem(Tq, Tk, dtype, 3)
    allowed = AR.allowed_mask(Tq, Tk, True)
    for wrong in (np.tril(np.ones((Tq, Tk), bool), -1), np.tril(np.ones((Tq, Tk), bool), 1)):  # j < i; j <= i + 1
        f = AR.fwd_ref(q, k, v, allowed, dtype)
        out, lse = AR.emu_fwd(q, k, v, wrong, dtype)
        _rejects(AR.check, out, f["O"], f["bound_O"], "out, causal off by one")
        _rejects(AR.check_lse, lse, f["lse"], f["bound_lse"], "lse, causal off by one")
        out, lse = AR.emu_fwd(q, k, v, allowed, dtype)
        b = AR.bwd_ref(q, k, v, do, allowed, dtype, out=out, lse=lse)
        got = AR.emu_bwd(q, k, v, out, do, lse, wrong, dtype)
        for g, n in zip(got, ("dQ", "dK", "dV")):
            _rejects(AR.check, g, b[n], b["bound_" + n], n + ", causal off by one")


@pytest.mark.parametrize("dtype", AC.DTYPES)
def test_rejects_dk_dv_without_the_last_query_block(dtype):
    Tq, Tk = 130, 130  # the last 64-query block holds two rows
    q, k, v, do = problem(Tq, Tk, dtype, 4)
    allowed = AR.allowed_mask(Tq, Tk, True)
    out, lse = AR.emu_fwd(q, k, v, allowed, dtype, block=64)
    b = AR.bwd_ref(q, k, v, do, allowed, dtype, out=out, lse=lse)
    got = AR.emu_bwd(q, k, v, out, do, lse, allowed, dtype, block=64, defect="drop_last_q_block")
    AR.check(got[0], b["dQ"], b["bound_dQ"], "dQ (not affected)")
    _rejects(AR.check, got[1], b["dK"], b["bound_dK"], "dK, last query block missing")
    _rejects(AR.check, got[2], b["dV"], b["bound_dV"], "dV, last query block missing")


@pytest.mark.parametrize("dtype", AC.DTYPES)
def test_rejects_a_skipped_rescale(dtype):
    Tq, Tk = 65, 200
    q, k, v, _ = problem(Tq, Tk, dtype, 6, qscale=4.0)
    k[Tk - 2] *= 3.0
    allowed = AR.allowed_mask(Tq, Tk)
    f = AR.fwd_ref(q, k, v, allowed, dtype)
    out, lse = AR.emu_fwd(q, k, v, allowed, dtype, block=64, defect="no_alpha")
    _rejects(AR.check, out, f["O"], f["bound_O"], "out, alpha skipped")
    _rejects(AR.check_lse, lse, f["lse"], f["bound_lse"], "lse, alpha skipped")


@pytest.mark.parametrize("dtype", AC.DTYPES)
def test_rejects_decode_reading_its_own_row_for_one_slot(dtype):
    R, H, L, cur = 5, 2, 64, 40
    q, kc, vc, src = _decode_problem(dtype, R, H, L, 7)
    src[:, 1] = (np.arange(R) + 1) % R  # slot 1 never lives in the row's own cache row
    ref, bound = AR.decode_ref(q, kc, vc, H, L, cur, dtype, src_row=src)
    _rejects(AR.check, AR.emu_decode(q, kc, vc, H, L, cur, dtype, src_row=src, defect="own_row_slot"), ref, bound, "decode, own row")


def _packed_lse(lse_rows, H, Tq_max, stride_of):
    """the packed forward's lse buffer [B][H][Tq_max] (canary-filled torch fp32) with sequence b's rows at ((b H + h) stride + i)"""
    import torch

    B = len(lse_rows)
    buf = GR.sentinel_fill(torch.empty(B * H * Tq_max + 8, dtype=torch.float32))
    for b, rows in enumerate(lse_rows):
        for h in range(H):
            o = (b * H + h) * stride_of(b)
            buf[o:o + len(rows[h])] = torch.from_numpy(np.asarray(rows[h], np.float32))
    return buf


def _lse_written(q_len, H, Tq_max, extra=8):
    import torch

    w = torch.zeros(len(q_len), H, Tq_max, dtype=torch.bool)
    for b, n in enumerate(q_len):
        w[b, :, :n] = True
    return torch.cat([w.reshape(-1), torch.zeros(extra, dtype=torch.bool)])


def test_rejects_packed_lse_indexed_with_q_len_and_canaries_past_q_len():
    q_len, H, Tq_max = [9, 33, 40], 2, 40
    refs, bounds, rows = [], [], []
    for b, n in enumerate(q_len):
        r = [problem(n, n, "bf16", 10 * b + h) for h in range(H)]
        f = [AR.fwd_ref(q, k, v, AR.allowed_mask(n, n, True), "bf16") for q, k, v, _ in r]
        rows.append([AR.emu_fwd(q, k, v, AR.allowed_mask(n, n, True), "bf16")[1] for q, k, v, _ in r])
        refs.append([x["lse"] for x in f])
        bounds.append([x["bound_lse"] for x in f])
    written = _lse_written(q_len, H, Tq_max)

    def verify(buf):
        AR.check_canary_mask(buf, written, "packed lse")
        t = buf[: len(q_len) * H * Tq_max].reshape(len(q_len), H, Tq_max).double().numpy()
        for b, n in enumerate(q_len):
            for h in range(H):
                AR.check_lse(t[b, h, :n], refs[b][h], bounds[b][h], f"packed lse b={b} h={h}")

    verify(_packed_lse(rows, H, Tq_max, lambda b: Tq_max))
    _rejects(verify, _packed_lse(rows, H, Tq_max, lambda b: q_len[b]))
    # lse[b][h][i], i >= q_len[b], is not written: a store there trips the canary
    buf = _packed_lse(rows, H, Tq_max, lambda b: Tq_max)
    buf[(0 * H + 1) * Tq_max + q_len[0]] = 0.0
    _rejects(verify, buf)


def test_canary_sees_one_row_past_a_packed_output():
    import torch

    total, cols, ld = 9 + 33 + 40, 128, 136
    alloc = GR.sentinel_fill(torch.empty(total + 3, ld, dtype=torch.bfloat16))
    alloc[:total, :cols] = 1.0
    GR.check_canary(alloc, (total, cols))
    alloc[total, 5] = 1.0  # the row after the last sequence's q_len rows
    with pytest.raises(AssertionError):
        GR.check_canary(alloc, (total, cols))


# ---------------------------------------------------------------------------------------------------------- dispatch and coverage
@pytest.mark.parametrize("name", [c["name"] for c in AC.ALL])
def test_case_reaches_the_kernel_it_claims(name):
    c = AC.BY_NAME[name]
    assert AC.dispatch_of(c) == c["claim"], (AC.dispatch_of(c), c["claim"])
    if "q_len" in c:
        assert max(c["q_len"]) <= c["Tq_max"] <= 64 and c["Tk"] <= 64 and (not c["kv_packed"] or c["Tk"] == c["Tq_max"])


def test_table_covers_every_dispatch_branch():
    claims = {c["claim"] for c in AC.ALL}
    assert claims == {"single", "tiled", "probs", "group2", "group4", "group8", "row", "chunked"}
    dec = AC.DECODE
    assert any(c["claim"] == "row" and c["row_div"] == 3 for c in dec)                                  # row_div without a group kernel
    assert any(c["claim"] == "row" and c["row_div"] == 4 and c["R"] % 4 for c in dec)                   # R % row_div != 0
    assert any(c["claim"] == "chunked" and c["row_div"] == 4 and not c["src"] for c in dec)            # group shape, > 64 slots
    assert {min(c["cur"] + 1, c["max_len"]) for c in dec if c["src"]} >= {1, 8, 63, 64, 65, 128, 200}
    assert any(c["cur"] + 1 > c["max_len"] for c in dec) and {c["ldc2"] for c in dec} == {False, True}
    d = AC.DENSE
    assert any(c["causal"] and c["Tq"] <= 64 < c["Tk"] for c in d) and any(c["causal"] and c["Tq"] > 64 >= c["Tk"] for c in d)
    assert any(c["causal"] and c["Tq"] != c["Tk"] and c["claim"] == "single" for c in d)
    assert {c["mask"] for c in d} >= {None, "suffix", "holes", "key0", "first_block", "middle_block", "nokey"}


def _instantiations(path):
    with open(os.path.join(ROOT, path)) as f:
        return {re.sub(r"\s+", "", m) for m in re.findall(r"(?:attn_[a-z_]*kernel|kv_append_kernel)<[^>]*>", f.read())}


def test_coverage_of_the_build_and_the_product_profiles():
    """the GPU module's committed kernel trace launches every attention instantiation the cases claim, every attn_* / kv_append
    kernel of the build's resource table and of the product's committed profiles — all but the fp8-emitting backward, which
    tests/test_fp8_conformance_gpu.py checks against the fp64 reference used here"""
    ns = lambda names: {re.sub(r"\s+", "", n) for n in names}  # noqa: E731
    traced = _instantiations(COVERAGE_PROFILE)
    claimed = ns(k for c in AC.ALL for dt in AC.DTYPES for k in AC.kernels_of(c["claim"], dt)) | ns(k for dt in AC.DTYPES for k in AC.kernels_of("kv_append", dt))
    assert claimed <= traced, sorted(claimed - traced)
    table = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_resources.json")))
    built = ns(k for unit in table.values() for k in unit if k.startswith("attn_") or k.startswith("kv_append"))
    assert len(built) >= 25
    assert built - ns([Q8_KERNEL]) <= traced, sorted(built - traced)
    prod = set().union(*(_instantiations(p) for p in PRODUCT_PROFILES))
    assert len(prod) >= 5
    assert prod - ns([Q8_KERNEL]) <= traced, sorted(prod - traced)


# ------------------------------------------------------------------------------ the emulations on the table's own operands
def _emu_problem(tag, what, dtype, q, k, v, do, allowed, block):
    out, lse = AR.emu_fwd(q, k, v, allowed, dtype, block=block)
    f = AR.fwd_ref(q, k, v, allowed, dtype)
    AR.check(out, f["O"], f["bound_O"], f"{tag} out: {what}")
    AR.check_lse(lse, f["lse"], f["bound_lse"], f"{tag} lse: {what}")
    got = AR.emu_bwd(q, k, v, out, do, lse, allowed, dtype, block=block)
    b = AR.bwd_ref(q, k, v, do, allowed, dtype, out=out, lse=lse)
    e = AR.bwd_ref(q, k, v, do, allowed, dtype)
    for g, n in zip(got, ("dQ", "dK", "dV")):
        assert np.isfinite(g).all()
        AR.check(g, b[n], b["bound_" + n], f"{tag} {n}: {what}")
        AR.check(g, e[n], e["bound_" + n], f"{tag} {n} end to end: {what}")


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in AC.DENSE])
def test_emulation_within_bounds_on_the_dense_cases(name, dtype):
    """the first and the last (batch, head) of every dense case, and every batch entry a 'nokey' mask touches.  The printed ratios
    are the emulation's column of profiles/attn_conformance_worst_ratio.txt."""
    c = AC.BY_NAME[name]
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    q, k, v, do, km = AC.dense_inputs(c, dtype)
    for b, h in sorted({(0, 0), (B - 1, H - 1), (1 % B, 0), (2 % B, H - 1)}):
        cs = slice(h * 64, (h + 1) * 64)
        allowed = AR.allowed_mask(Tq, Tk, c["causal"], km[b] if km is not None else None)
        _emu_problem(f"{c['claim']}/{dtype}", name, dtype, q[b * Tq:(b + 1) * Tq, cs], k[b * Tk:(b + 1) * Tk, cs], v[b * Tk:(b + 1) * Tk, cs],
                     do[b * Tq:(b + 1) * Tq, cs], allowed, 64 if c["claim"] == "tiled" else None)


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in AC.PACKED])
def test_emulation_within_bounds_on_the_packed_cases(name, dtype):
    c = AC.BY_NAME[name]
    q, k, v, do, q_off = AC.packed_inputs(c, dtype)
    cs = slice((c["H"] - 1) * 64, c["H"] * 64)
    for b, n in enumerate(c["q_len"]):
        r = slice(int(q_off[b]), int(q_off[b]) + n)
        rk = r if c["kv_packed"] else slice(b * c["Tk"], (b + 1) * c["Tk"])
        _emu_problem(f"packed/{dtype}", f"{name} b={b}", dtype, q[r, cs], k[rk, cs], v[rk, cs], do[r, cs],
                     AR.allowed_mask(n, rk.stop - rk.start, c["causal"]), None)


@pytest.mark.parametrize("dtype", AC.DTYPES)
@pytest.mark.parametrize("name", [c["name"] for c in AC.DECODE])
def test_emulation_within_bounds_on_the_decode_cases(name, dtype):
    c = AC.BY_NAME[name]
    q, kc, vc, src = AC.decode_inputs(c, dtype)
    ref, bound = AR.decode_ref(q, kc, vc, c["H"], c["max_len"], c["cur"], dtype, src_row=src, row_div=c["row_div"])
    got = AR.emu_decode(q, kc, vc, c["H"], c["max_len"], c["cur"], dtype, src_row=src, row_div=c["row_div"])
    AR.check(got, ref, bound, f"decode_{c['claim']}/{dtype} out: {name}")
