"""Decode selection conformance on the MI355X: the kernels of csrc/decode.hip that pick the next token in generate() —
mic_row_lse_topk, mic_row_forced_topk, mic_row_topk_tiles, mic_warp_thresholds, mic_sample_rows, mic_greedy_step — on every case of
tests/util_decode_cases.py, in bf16 and fp32 where the entry point takes a dtype, against the fp64 references of
tests/util_decode_ref.py.  Every case is admissible (tests/test_decode_conformance_cpu.py asserts it), so the demands are exact: the
reference's index sequence, values within the derived bound (bit for bit where the reference is exact), equal isfinite patterns,
indices distinct and < V; the keep mask of the fp64 warpers; the reference's draw.  Around every call:
  - outputs are windows in canary-filled allocations and every element outside the window keeps its bits;
  - logit columns V .. ld, rows past R and stat entries past ntiles hold NaN;
  - each launch runs twice from refilled outputs and gives identical bits (nothing here depends on atomic order for its result).
Out of scope: mic_beam_step / mic_beam_step_groups (their own suite: tests/test_beam_conformance_gpu.py, every search step against
the oracle's loop body), the _q8 kernels."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_decode_cases as DC  # noqa: E402
import util_decode_ref as DR  # noqa: E402
import util_rowop_ref as RR  # noqa: E402
from test_attn_conformance_gpu import TD, Buf, _refused  # noqa: E402
from test_rowop_conformance_gpu import put1, twice, vec  # noqa: E402

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
CANARY_I32 = -1515870811  # 0xA5A5A5A5


class IBuf:
    """Buf for int32: a [rows][cols] window (row stride cols) 4 elements into a canary-filled allocation with 3 rows and 8 elements
    behind it"""

    def __init__(self, rows, cols, dev, off=4, extra=3):
        self.rows, self.cols, self.ld, self.off = rows, cols, cols, off
        self.flat = torch.empty(off + (rows + extra) * cols + 8, dtype=I32, device=dev)
        self.full = self.flat[off:off + (rows + extra) * cols].view(rows + extra, cols)
        self.t = self.full[:rows]
        self.refill()

    def refill(self):
        self.flat.fill_(CANARY_I32)
        return self

    def put(self, x):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(x)).to(I32).reshape(self.rows, self.cols))
        return self

    def get(self):
        return self.t.cpu().numpy().astype(np.int64)

    def bits(self):
        return self.flat.clone()

    def check_canary(self, what, written=None):
        c = self.flat.clone()
        win = c[self.off:self.off + self.full.numel()].view(self.full.shape)[:self.rows]
        if written is None:
            win[...] = CANARY_I32
        else:
            win[written.to(torch.bool).to(c.device)] = CANARY_I32
        bad = (c != CANARY_I32).nonzero()
        assert bad.numel() == 0, f"{what}: {bad.numel()} int32 elements outside the window written, first at flat index {bad[0].item()}"


def refused(fn, outs, what, entry):
    """_refused, and mic_last_error holds a message of that entry point"""
    from mic_amd import _lib as L

    def run():
        try:
            fn()
        except L.MicError:
            msg = L.lib().mic_last_error().decode()
            assert msg.startswith(entry + ":"), f"{what}: mic_last_error is {msg!r}"
            raise

    _refused(run, outs, what)


def report(quantity, case, worst, n):
    print(f"[conformance] {quantity}: {case}: worst err/bound {worst:.3g} over {n} elements")


def bias_vec(bias, dev):
    return put1(vec(len(bias), dev, "nan"), bias)


# ------------------------------------------------------------------------------------------------ mic_row_lse_topk
@functools.lru_cache(maxsize=None)
def _lse_case(V, rows, mode):
    """the inputs and the fp64 reference rows, computed once and shared by both storage types"""
    x0, bias = DC.lse_grid_rows(V) if rows == "grid" else DC.lse_edge_rows(V)
    x, sup, eos, raw = DC.lse_mode(x0, mode)
    return x, bias, sup, eos, raw, [DR.proc_ref(x[r], bias[r], suppress_eos=sup, eos=eos, raw=raw) for r in range(x.shape[0])]


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V", DC.LSE_V)
def test_row_lse_topk(dev, V, dtype):
    """plain mode: every k with both row strides; raw / suppress_eos modes: k = 1, a middle one and the widest, the strides alternating"""
    from mic_amd import ops

    dt, ks, lds = TD[dtype], DC.lse_ks(V), DC.lse_lds(V)
    for rows in ("grid", "edge"):
        names = DC.BIASES if rows == "grid" else DC.LSE_EDGE_ROWS
        for mi, mode in enumerate(DC.LSE_MODES):
            x, bias, sup, eos, raw, refs = _lse_case(V, rows, mode)
            R = x.shape[0]
            bd = bias_vec(bias, dev)
            lgs = {ld: Buf(R, V, ld, dt, dev, "nan").put(x) for ld in lds}
            runs = [(k, ld) for k in ks for ld in lds] if mode == "plain" else \
                   [(k, lds[(mi + j) % 2]) for j, k in enumerate(sorted({ks[0], ks[len(ks) // 2], ks[-1]}))]
            worst = [0.0] * R
            for k, ld in runs:
                tv, ti = Buf(R, k, k, F32, dev, "canary", off=4), IBuf(R, k, dev)
                what = f"V={V} ld={ld} k={k} {mode}"
                twice(lambda: ops.row_lse_topk(lgs[ld].t, ld, V, k, tv.t, ti.t, R, suppress_eos=sup, eos_token_id=eos, raw_logits=raw, row_bias=bd.t[0]),
                      [tv, ti], what)
                tv.check_canary(what)
                ti.check_canary(what)
                gv, gi = tv.get(), ti.get()
                for r in range(R):
                    w = DR.check_topk(gv[r], gi[r], refs[r], k, V, f"{what} {names[r]}", "value", log=False)
                    worst[r] = max(worst[r], w or 0.0)
            for r in range(R):
                if not refs[r]["exact"]:
                    report(f"row_lse_topk/{dtype} value", f"V={V} {mode} {names[r]}", worst[r], sum(k for k, _ in runs))


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V", DC.LSE_V)
def test_row_lse_topk_forced(dev, V, dtype):
    """the forced branch (ForcedBOS / ForcedEOS) with the token at 0, in the middle and at V - 1: exactly the reference's top-k of
    'everything -inf, the forced token 0', + the row's bias; the logits (all NaN here) are not read"""
    from mic_amd import ops

    ks = DC.lse_ks(V)
    bias = np.array(DC.BIASES)
    R, bd, ld = 4, bias_vec(bias, dev), DC.lse_lds(V)[1]
    lg = Buf(R, V, ld, TD[dtype], dev, "nan")
    for forced in (0, V // 2, V - 1):
        for k in sorted({ks[0], ks[len(ks) // 2], ks[-1]}):
            tv, ti = Buf(R, k, k, F32, dev, "canary", off=4), IBuf(R, k, dev)
            what = f"V={V} k={k} forced={forced}"
            twice(lambda: ops.row_lse_topk(lg.t, ld, V, k, tv.t, ti.t, R, forced_token=forced, row_bias=bd.t[0]), [tv, ti], what)
            tv.check_canary(what)
            ti.check_canary(what)
            for r in range(R):
                rv, ri = DR.forced_ref(V, forced, k, bias[r])
                assert np.array_equal(ti.get()[r], ri) and np.array_equal(tv.get()[r], rv), f"{what} row {r}"


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("k", DC.FORCED_K)
def test_row_forced_topk(dev, k, with_bias):
    from mic_amd import ops

    ids = DC.FORCED_ROWS
    R = ids.size
    bias = np.array([0.0, -3.5, 2.0, -1e7, 0.25, -0.0])
    fd, bd = torch.from_numpy(ids).to(dev), bias_vec(bias, dev)
    tv, ti = Buf(R, k, k, F32, dev, "canary", off=4), IBuf(R, k, dev)
    twice(lambda: ops.row_forced_topk(R, k, fd, tv.t, ti.t, row_bias=bd.t[0] if with_bias else None), [tv, ti], f"forced k={k}")
    tv.check_canary("top_val")
    ti.check_canary("top_idx")
    for r in range(R):
        rv, ri = DR.forced_ref(int(max(ids.max(), k)) + 2, int(ids[r]), k, bias[r] if with_bias else 0.0)
        assert np.array_equal(ti.get()[r], ri) and np.array_equal(tv.get()[r], rv), f"forced k={k} row {r}"


# ------------------------------------------------------------------------------------------------ mic_row_topk_tiles
def stat_window(part, dev):
    """[R][ntiles][2] partials -> a [R][2 * stat_ld] view, stat_ld = ntiles + 3: entries ntiles .. stat_ld and a row behind hold NaN"""
    R, nt = part.shape[:2]
    stat_ld = nt + 3
    flat = torch.full(((R + 1) * 2 * stat_ld + 8,), float("nan"), dtype=F32, device=dev)
    st = flat[4:4 + R * 2 * stat_ld].view(R, 2 * stat_ld)
    st[:, :2 * nt] = torch.from_numpy(part.reshape(R, 2 * nt)).to(dev)
    return st


@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("k", DC.TILES_K)
def test_row_topk_tiles(dev, k, dtype):
    """the stats are built here in fp64 from the stored logits (the max exact, the sum rounded to fp32); the result equals the
    reference and mic_row_lse_topk on the same logits (same indices; both values within their bounds of the same fp64 value)"""
    from mic_amd import ops

    dt = TD[dtype]
    for nt in DC.tiles_ntiles(k):
        x, bias, eos = DC.tiles_rows(nt, k)
        R, V = x.shape
        part = RR.tile_partials(x)
        ld = DC.up8(V) + 8
        lg, st, bd = Buf(R, V, ld, dt, dev, "nan").put(x), stat_window(part, dev), bias_vec(bias, dev)
        for sup, raw in ((False, False), (True, False), (False, True)):
            what = f"ntiles={nt} k={k}{' suppress_eos' if sup else ''}{' raw' if raw else ''}"
            tv, ti = Buf(R, k, k, F32, dev, "canary", off=4), IBuf(R, k, dev)
            kw = dict(suppress_eos=sup, eos_token_id=eos, raw_logits=raw, row_bias=bd.t[0])
            twice(lambda: ops.row_topk_tiles(lg.t, ld, V, st, k, tv.t, ti.t, R, **kw), [tv, ti], what)
            tv.check_canary(what)
            ti.check_canary(what)
            sv, si = Buf(R, k, k, F32, dev, "canary", off=4), IBuf(R, k, dev)
            ops.row_lse_topk(lg.t, ld, V, k, sv.t, si.t, R, **kw)
            same = [r for r in range(R) if not (raw and k == 1 and abs(bias[r]) >= DR.BIG_BIAS)]  # (there the streaming kernel is the
            assert np.array_equal(si.get()[same], ti.get()[same]), f"{what}: mic_row_lse_topk picks other indices"   # argmax of the logits)
            for r in range(R):
                ref = DR.proc_ref(x[r], bias[r], suppress_eos=sup, eos=eos, raw=raw, part=part[r])
                w = DR.check_topk(tv.get()[r], ti.get()[r], ref, k, V, f"{what} row {r}", "value", log=False)
                if w is not None:
                    report(f"row_topk_tiles/{dtype} value", f"{what} row {r}", w, k)
                if raw and r in same:
                    assert np.array_equal(sv.get()[r], tv.get()[r]), f"{what} row {r}: raw values differ from mic_row_lse_topk"


# ------------------------------------------------------------------------------------------------ mic_warp_thresholds
@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V", DC.WARP_V)
def test_warp_thresholds(dev, V, dtype):
    """the keep mask rebuilt from (thr, tie_limit) equals the fp64 warpers' mask, and holds min(k, finite) entries after top-k"""
    from mic_amd import ops

    x = DC.warp_rows(V, dtype)
    R, ld = x.shape[0], V + 3
    lg = Buf(R, V, ld, TD[dtype], dev, "nan").put(x)
    thr, lim = vec(R, dev), IBuf(1, R, dev)
    for (k, p, T, sup) in DC.warp_combos(V):
        what = f"V={V} top_k={k} top_p={p} T={T} suppress={sup}"
        twice(lambda: ops.warp_thresholds(lg.t, ld, V, thr.t[0], lim.t[0], R, temperature=T, suppress_eos=sup, eos_token_id=2, top_k=k, top_p=p),
              [thr, lim], what)
        thr.check_canary(what)
        lim.check_canary(what)
        gt, gl = thr.get()[0], lim.get()[0]
        for r in range(R):
            y = DR.scaled(x[r], T, sup, 2)
            ref = DR.warp_ref(y, k, p)
            got = DR.mask_of(y, gt[r], gl[r])
            assert np.array_equal(got, ref["keep"]), f"{what} {DC.WARP_ROWS[r]}: keeps {int(got.sum())}, the warpers {int(ref['keep'].sum())} (thr {gt[r]!r} tie_limit {gl[r]})"
            if k > 0 and p >= 1.0:
                assert got.sum() == min(k, int(np.isfinite(y).sum())), what
            assert not (gt[r] == 0 and np.signbit(gt[r])), f"{what}: thr is -0"


@pytest.mark.parametrize("dtype", DC.DTYPES)
def test_signed_zero_example(dev, dtype):
    """[+0, -0, -0, +0, -1]: top_k = 3 keeps three tokens (the first three zeros), top_p = 0.6 three as well; mic_sample_rows under
    those thresholds draws what the reference draws"""
    from mic_amd import ops
    from oracle import generation_ref as G

    x = DC.ZERO_ROW[None]
    lg = Buf(1, 5, 8, TD[dtype], dev, "nan").put(x)
    assert torch.equal(torch.signbit(lg.t[0].float()).cpu(), torch.tensor([False, True, True, False, True]))
    thr, lim, out = vec(1, dev), IBuf(1, 1, dev), IBuf(1, 1, dev)
    y = DR.scaled(x[0], 1.0)
    for k, p in ((3, 1.0), (0, 0.6)):
        twice(lambda: ops.warp_thresholds(lg.t, 8, 5, thr.t[0], lim.t[0], 1, top_k=k, top_p=p), [thr, lim], "signed zeros")
        got = DR.mask_of(y, thr.get()[0, 0], lim.get()[0, 0])
        assert got.tolist() == [True, True, True, False, False] == DR.warp_ref(y, k, p)["keep"].tolist(), (k, p, got)
        for seed in range(6):
            key = G.prng_split(G.prng_key(seed))[0]
            ref, ok, _ = DR.sample_ref(x, key, thr=thr.get()[0].astype(np.float32), lim=lim.get()[0])
            twice(lambda: ops.sample_rows(lg.t, 8, 5, key, out.t[0], 1, min_keep=thr.t[0], tie_limit=lim.t[0]), [out], "signed zeros")
            assert ok[0] and out.get()[0, 0] == ref[0] and ref[0] < 3, (k, p, seed)


# ------------------------------------------------------------------------------------------------ mic_sample_rows
@pytest.mark.parametrize("dtype", DC.DTYPES)
@pytest.mark.parametrize("V", DC.SAMPLE_V)
@pytest.mark.parametrize("R", DC.SAMPLE_R)
def test_sample_rows(dev, R, V, dtype):
    from mic_amd import ops
    from oracle import generation_ref as G

    x = DC.sample_rows_of(R, V)
    ld = V + 5
    lg = Buf(R, V, ld, TD[dtype], dev, "nan").put(x)
    key = G.prng_split(G.prng_key(DC.SAMPLE_KEY_SEED.get((R, V), R + V)))[0]
    out = IBuf(1, R, dev)
    for variant in DC.SAMPLE_VARIANTS:
        s = DR.sample_setup(x, variant)
        ref, ok, info = DR.sample_ref(x, key, **s)
        assert all(ok), info
        td = put1(vec(R, dev, "nan"), s["thr"]) if s["thr"] is not None else None
        ldv = torch.from_numpy(s["lim"]).to(dev) if s["lim"] is not None else None
        what = f"R={R} V={V} {variant}"
        twice(lambda: ops.sample_rows(lg.t, ld, V, key, out.t[0], R, temperature=s["temperature"], suppress_eos=s["suppress_eos"], eos_token_id=s["eos"],
                                      min_keep=td.t[0] if td else None, tie_limit=ldv), [out], what)
        out.check_canary(what)
        assert np.array_equal(out.get()[0], ref), f"{what}: drew {out.get()[0].tolist()}, the reference {ref.tolist()}"
    forced = V - 1
    twice(lambda: ops.sample_rows(lg.t, ld, V, key, out.t[0], R, forced_token=forced), [out], "forced")
    out.check_canary("forced")
    assert (out.get()[0] == forced).all()


# ------------------------------------------------------------------------------------------------ mic_greedy_step
@pytest.mark.parametrize("ld_top", DC.GREEDY_LD)
@pytest.mark.parametrize("B", DC.GREEDY_B)
def test_greedy_step(dev, B, ld_top):
    """rows already finished, rows finishing now (the EOS step writes PAD) and rows running; only column cur_len of sequences moves"""
    from mic_amd import ops

    L, eos, pad = 6, 2, 1
    b = np.arange(B)
    fin0 = (b % 3 == 0).astype(np.int32)
    top = np.full((B, ld_top), 77, np.int32)
    top[:, 0] = np.where(b % 3 == 1, eos, b + 5)
    topd = torch.from_numpy(top).to(dev)
    seq, fin, nxt = IBuf(B, L, dev), IBuf(1, B, dev), IBuf(1, B, dev)
    for cur in (1, L - 1):
        twice(lambda: ops.greedy_step(B, L, cur, eos, pad, topd, ld_top, seq.t, fin.t[0], nxt.t[0]), [seq, fin, nxt], f"greedy B={B}",
              prep=lambda: fin.put(fin0))
        col = torch.zeros(B, L, dtype=torch.bool)
        col[:, cur] = True
        seq.check_canary("sequences outside column cur_len", col)
        fin.check_canary("finished")
        nxt.check_canary("next_token")
        rs, rf, rt = DR.greedy_ref(top[:, 0], np.zeros((B, L), np.int64), fin0, cur, eos, pad)
        assert np.array_equal(seq.get()[:, cur], rs[:, cur]) and np.array_equal(fin.get()[0], rf) and np.array_equal(nxt.get()[0], rt)
        assert (rt[b % 3 != 2] == pad).all() and (rt[b % 3 == 2] == b[b % 3 == 2] + 5).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_decode_refusals(dev):
    """every MIC_CHECK of the entry points in scope: non-zero, mic_last_error set, nothing written.  All of them are tested before any
    launch by the host code"""
    from mic_amd import _lib as L
    from mic_amd import ops

    R, V, ld, k = 2, 40, 48, 4
    for dtype in DC.DTYPES:
        lg = Buf(R, V, ld, TD[dtype], dev, "nan").put(np.zeros((R, V)))
        tv, ti = Buf(R, 80, 80, F32, dev, "canary", off=4), IBuf(R, 80, dev)
        o = [tv, ti]
        top = lambda **kw: ops.row_lse_topk(lg.t, kw.pop("ld", ld), kw.pop("V", V), kw.pop("k", k), kw.pop("tv", tv.t), ti.t, R, **kw)  # noqa: E731
        n = "mic_row_lse_topk"
        refused(lambda: top(k=0), o, "k 0", n)
        refused(lambda: top(k=65), o, "k 65", n)
        refused(lambda: top(k=41), o, "k > V", n)
        refused(lambda: top(V=7, ld=8, k=8), o, "k > V at V 7", n)
        refused(lambda: top(k=41, forced_token=3), o, "k > V, forced", n)
        refused(lambda: top(forced_token=40), o, "forced_token = V", n)
        refused(lambda: top(ld=32), o, "ld < V", n)
        refused(lambda: top(V=36, ld=44), o, "ld % 8", n)
        refused(lambda: top(tv=None), o, "top_val NULL", n)
        refused(lambda: L.check(L.lib().mic_row_lse_topk(9, R, V, lg.t.data_ptr(), ld, k, -1, 0, 2, 0, None, tv.t.data_ptr(), ti.t.data_ptr(), None),
                                n), o, "dtype 9", n)
        st = torch.zeros(R, 2 * 4, device=dev)
        tiles = lambda **kw: ops.row_topk_tiles(lg.t, kw.pop("ld", ld), kw.pop("V", V), kw.pop("st", st), kw.pop("k", k), tv.t, kw.pop("ti", ti.t), R, **kw)  # noqa: E731
        n = "mic_row_topk_tiles"
        refused(lambda: tiles(k=0), o, "k 0", n)
        refused(lambda: tiles(k=17), o, "k 17", n)
        refused(lambda: tiles(V=7, ld=8, k=8), o, "k > V", n)
        refused(lambda: tiles(ld=32), o, "ld < V", n)
        refused(lambda: tiles(V=262145, ld=262152, st=torch.zeros(1, 2 * 4100, device=dev)), o, "V > 262144", n)
        refused(lambda: tiles(V=300, ld=304), o, "stat_ld < ntiles", n)
        refused(lambda: tiles(ti=None), o, "top_idx NULL", n)
        refused(lambda: L.check(L.lib().mic_row_topk_tiles(9, R, V, lg.t.data_ptr(), ld, st.data_ptr(), 4, k, 0, 2, 0, None, tv.t.data_ptr(),
                                                           ti.t.data_ptr(), None), n), o, "dtype 9", n)
        thr, lim, out = vec(R, dev), IBuf(1, R, dev), IBuf(1, R, dev)
        warp = lambda **kw: ops.warp_thresholds(lg.t, kw.pop("ld", ld), V, kw.pop("thr", thr.t[0]), lim.t[0], R, **kw)  # noqa: E731
        n = "mic_warp_thresholds"
        refused(lambda: warp(temperature=0.0), [thr, lim], "temperature 0", n)
        refused(lambda: warp(temperature=-1.0), [thr, lim], "temperature < 0", n)
        refused(lambda: warp(top_p=0.0), [thr, lim], "top_p 0", n)
        refused(lambda: warp(ld=32), [thr, lim], "ld < V", n)
        refused(lambda: warp(thr=None), [thr, lim], "thr NULL", n)
        refused(lambda: L.check(L.lib().mic_warp_thresholds(9, R, V, lg.t.data_ptr(), ld, 1.0, 0, 2, 3, 0.5, thr.t.data_ptr(), lim.t.data_ptr(), None), n),
                [thr, lim], "dtype 9", n)
        samp = lambda **kw: ops.sample_rows(lg.t, kw.pop("ld", ld), kw.pop("V", V), (1, 2), kw.pop("out", out.t[0]), kw.pop("R", R), **kw)  # noqa: E731
        n = "mic_sample_rows"
        refused(lambda: samp(temperature=0.0), [out], "temperature 0", n)
        refused(lambda: samp(ld=32), [out], "ld < V", n)
        refused(lambda: samp(forced_token=V), [out], "forced_token = V", n)
        refused(lambda: samp(R=65536, V=65536, ld=65536), [out], "R * V = 2^32", n)
        refused(lambda: samp(out=None), [out], "out NULL", n)
        refused(lambda: L.check(L.lib().mic_sample_rows(9, R, V, lg.t.data_ptr(), ld, 1, 2, 1.0, -1, 0, 2, None, None, out.t.data_ptr(), None), n),
                [out], "dtype 9", n)
    fd = torch.zeros(R, dtype=I32, device=dev)
    n = "mic_row_forced_topk"
    refused(lambda: ops.row_forced_topk(R, 0, fd, tv.t, ti.t), o, "k 0", n)
    refused(lambda: ops.row_forced_topk(R, 65, fd, tv.t, ti.t), o, "k 65", n)
    refused(lambda: ops.row_forced_topk(R, 4, None, tv.t, ti.t), o, "forced_rows NULL", n)
    seq, fin, nxt = IBuf(R, 6, dev), IBuf(1, R, dev), IBuf(1, R, dev)
    n = "mic_greedy_step"
    refused(lambda: ops.greedy_step(R, 6, 0, 2, 1, fd, 1, seq.t, fin.t[0], nxt.t[0]), [seq, fin, nxt], "cur_len 0", n)
    refused(lambda: ops.greedy_step(R, 6, 6, 2, 1, fd, 1, seq.t, fin.t[0], nxt.t[0]), [seq, fin, nxt], "cur_len = max_len", n)
    refused(lambda: ops.greedy_step(R, 6, 1, 2, 1, None, 1, seq.t, fin.t[0], nxt.t[0]), [seq, fin, nxt], "top_idx NULL", n)
