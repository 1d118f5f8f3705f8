"""GEMM conformance on the MI355X: every case of tests/util_gemm_cases.py (the kernel instantiations the product launches, at
its shapes, plus every epilogue feature the header admits and the ragged edges) against the fp64 reference of
tests/util_gemm_ref.py, element-wise on sampled rows and columns (full K).  Around every call:
  - outputs (C, Zout, a_rowsum, rowstat, rowsum2, split-K slabs) sit in larger allocations filled with a NaN-payload canary, with
    extra rows and ld > N; every element outside the window must keep its bits;
  - the operands' padding (past K inside lda, past M / N inside the allocation) holds NaN, and the rows [k_valid, K) of both
    k-major operands hold NaN and +-3e38: a NaN or overflow that reaches a valid output fails the comparison;
  - non-atomic paths run twice and must give identical bits.
The plan each case claims is asserted against mic_gemm_plan on the real arguments.  The library latches its A/B switches at the
first GEMM, so the switch configurations rerun the cases they can change in child processes, one after another."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_gemm_cases as GC  # noqa: E402
import util_gemm_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu

FP8 = {"e4m3": (torch.float8_e4m3fn, 448.0), "e5m2": (torch.float8_e5m2, 57344.0)}
DROP_SEED = 0x5EED


def _nanfill(t):
    if t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        t.view(torch.uint8).fill_(0x7F)
    else:
        t.fill_(float("nan"))
    return t


def _operand(rows, cols, ld, dtype, gen, dev, *, pad_rows=16, stale_from=None, mean=None, scale=1.0):
    """[rows][cols] of randn values inside a NaN-filled [rows + pad_rows][ld] allocation (bf16, or fp8 bytes under a per-tensor
    scale: then also returns scale_inv).  Rows >= stale_from (the k-major operands' [k_valid, K)) hold NaN and +-3e38."""
    x = torch.randn(rows, cols, generator=gen, device=dev) * scale
    if mean is not None:
        x += mean[:, None]
    fp8 = dtype in FP8
    buf = _nanfill(torch.empty(rows + pad_rows, ld, dtype=FP8[dtype][0] if fp8 else torch.bfloat16, device=dev))
    sinv = None
    if fp8:
        amax = x.abs().max()
        q = (x * (FP8[dtype][1] / amax)).to(FP8[dtype][0])
        buf[:rows, :cols] = q
        sinv = (amax / FP8[dtype][1]).reshape(1).float()
    else:
        buf[:rows, :cols] = x.to(torch.bfloat16)
    if stale_from is not None and stale_from < rows:
        st = buf[stale_from:rows, :cols]
        if fp8:
            st.view(torch.uint8)[:, 0::2] = 0x7F
            st.view(torch.uint8)[:, 1::2] = 0xFF
        else:
            st[:, 0::3] = float("nan")
            st[:, 1::3] = 3e38
            st[:, 2::3] = -3e38
    return buf, sinv


def _deq(t, sinv):
    v = t.float().double()
    return v * float(sinv.item()) if sinv is not None else v


def _padded(rows, ld, dev, off):
    """a NaN-filled bf16 [rows][ld] input whose base address lies `off` elements past a 16-B boundary"""
    return _nanfill(torch.empty(rows * ld + 16, dtype=torch.bfloat16, device=dev))[off:off + rows * ld].view(rows, ld)


def _canary(shape, dtype, dev, off=0):
    n = int(np.prod(shape))
    flat = GR.sentinel_fill(torch.empty(n + 16, dtype=dtype, device=dev))
    return flat[off:off + n].view(*shape)


class Problem:
    """one GEMM problem of a case: device operands, outputs in canary allocations, the launch arguments and the reference check"""

    def __init__(self, c, M, N, K, f, gen, dev, idx):
        from mic_amd import ops

        self.c, self.M, self.N, self.K, self.f, self.dev = c, M, N, K, f, dev
        dt = c["dtype"]
        self.fp8 = dt != "bf16"
        akm, bkm = c["akm"], c["bkm"]
        kv = f.get("k_valid", 0)
        self.kv = kv
        stale = kv if (akm and bkm and kv) else None
        pad = 16 if self.fp8 else 8
        mean = None
        if f.get("ln"):  # rows with a mean of several sigma: the cancellation the folded LayerNorm has to survive
            mean = (torch.rand(M, generator=gen, device=dev) * 2 - 1) * 6
        if akm:
            self.A, self.sa = _operand(K, M, M + pad, dt, gen, dev, stale_from=stale)
        else:
            self.A, self.sa = _operand(M, K, K + pad, dt, gen, dev, mean=mean)
        bdt = "e4m3" if self.fp8 else dt
        bscale = 0.05 if f.get("ln") else 1.0
        if bkm:
            self.B, self.sb = _operand(K, N, N + pad, bdt, gen, dev, stale_from=stale, scale=bscale)
        else:
            self.B, self.sb = _operand(N, K, K + pad, bdt, gen, dev, scale=bscale)
        ld = GC.ld_of(N, f)
        self.ld = ld
        self.c8 = f.get("c8")  # fp8 C emission ("e4m3" / "e5m2") under a delayed scale
        self.c_dt = FP8[self.c8][0] if self.c8 else (torch.float32 if f.get("c32") else torch.bfloat16)
        off = 1 if f.get("off") else 0
        self.off = off
        kw = dict(a_kmajor=akm, b_kmajor=bkm, alpha=f.get("alpha", 1.0))
        self.bias = torch.randn(N, generator=gen, device=dev) if (f.get("bias") or f.get("ln")) else None
        kw["bias"] = self.bias
        kw["act"], kw["dact"] = f.get("act", 0), f.get("dact", 0)
        self.zin = None
        if f.get("dact"):
            self.zin = _padded(M + 8, ld, dev, off)
            self.zin[:M, :N] = (torch.randn(M, N, generator=gen, device=dev) * 1.5).to(torch.bfloat16)
            kw["zin"] = self.zin
        self.R = None
        if f.get("res"):
            self.R = _padded(M + 8, ld, dev, off)
            self.R[:M, :N] = (torch.randn(M, N, generator=gen, device=dev) * 4).to(torch.bfloat16)
            kw["residual"], kw["ldr"] = self.R, ld
        if f.get("zout") or f.get("dact"):
            kw["ldz"] = ld
        self.C_old = None
        if f.get("acc"):
            self.C_old = (torch.randn(M, N, generator=gen, device=dev) * 8).to(self.c_dt)
            kw["accumulate"] = True
        if f.get("drop"):
            kw["dropout_p"], kw["dropout_seed"] = f["drop"], DROP_SEED + idx
        if f.get("split"):
            kw["split_k"] = f["split"]
        if kv:
            kw["k_valid"] = kv
        if f.get("rowsum_k"):
            kw["rowsum_k"] = f["rowsum_k"]
        if self.fp8:
            kw["a_scale_inv"], kw["b_scale_inv"] = self.sa, self.sb
        if f.get("rowstat"):
            kw["rowstat_nvalid"] = f.get("nvalid", 0)
        self.ln = None
        if f.get("ln"):
            xa = self.A[:M, :K].double()
            st = torch.stack([xa.sum(1), (xa * xa).sum(1)], 1) * 2.0 ** 20
            self.ln_stats = st.round().to(torch.int64)
            self.ln_g = self.B[:N, :K].double().sum(1).float()
            kw.update(ln_stats=self.ln_stats, ln_colsum=self.ln_g, ln_width=K, ln_eps=1e-5)
        self.kw = kw
        self.outputs()

    def outputs(self):
        """(re)allocate every output in its canary allocation and (re)write the caller-initialised parts"""
        M, N, f, dev, ld, off = self.M, self.N, self.f, self.dev, self.ld, self.off
        kw = self.kw
        if f.get("slabs"):
            self.stride = (M * ld + 63) // 64 * 64
            self.ws = _canary((f["split"] * self.stride + 64,), torch.float32, dev)
            self.C = _canary((M + 8, ld), self.c_dt, dev, off)
            kw["split_stride"] = self.stride
        else:
            self.C = _canary((M + 8, ld), self.c_dt, dev, off)
            if f.get("split"):
                self.C[:M, :N] = 0
        if self.C_old is not None:
            self.C[:M, :N] = self.C_old
        if self.c8:  # the tensor's amax of the "previous pass": chosen so that the largest outputs saturate
            from mic_amd import ops

            self.q8_state = torch.tensor([f.get("c8_amax", 6.0), -1.0], device=dev)
            self.q8_amax = _canary((ops.fp8_amax_partials() + 16,), torch.float32, dev)
            self.q8_amax[:ops.fp8_amax_partials()] = 0
            kw["c_q8"] = (self.q8_state, self.q8_amax)
        self.Z = _canary((M + 8, ld), torch.bfloat16, dev, off) if f.get("zout") else None
        kw["zout"] = self.Z
        self.rs = None
        if f.get("rowsum"):
            self.rs = _canary((M + 16,), torch.float32, dev)
            self.rs[:M] = 0
        kw["a_rowsum"] = self.rs
        self.stat = None
        if f.get("rowstat"):
            self.stat = _canary((M + 4, N // 64 + 3, 2), torch.float32, dev)
        kw["rowstat"] = self.stat
        self.r2 = None
        if f.get("rowsum2"):
            self.r2 = _canary((M + 4, 2), torch.int64, dev)
            self.r2[:M] = 0
        kw["rowsum2"] = self.r2

    def args(self):
        from mic_amd import ops

        out = self.ws if self.f.get("slabs") else self.C
        kw = dict(self.kw)
        ldc = self.ld
        if self.f.get("slabs"):
            kw["split_stride"] = self.stride
        return ops.gemm_args(self.A, self.B, out, self.M, self.N, self.K, lda=self.A.stride(0), ldb=self.B.stride(0), ldc=ldc, **kw)

    def finish(self):
        from mic_amd import ops

        if self.f.get("slabs"):
            if self.N % 8 == 0 and self.ld % 8 == 0 and self.C.data_ptr() % 16 == 0:
                ops.sum_slabs(self.ws, self.f["split"], self.stride, self.C, self.M, self.N, self.ld, self.ld)
            else:  # the slabs in fixed order, fp32, as mic_sum_slabs adds them
                w = self.ws[:self.f["split"] * self.stride].view(self.f["split"], self.stride)[:, :self.M * self.ld]
                acc = w[0].clone()
                for s in range(1, self.f["split"]):
                    acc += w[s]
                self.C[:self.M, :self.N] = acc.view(self.M, self.ld)[:, :self.N]

    def check_canaries(self):
        M, N, f = self.M, self.N, self.f
        GR.check_canary(self.C, (M, N), "C")
        if self.Z is not None:
            GR.check_canary(self.Z, (M, N), "Zout")
        if self.rs is not None:
            GR.check_canary(self.rs, (slice(0, M),), "a_rowsum")
        if self.stat is not None:
            GR.check_canary(self.stat, (slice(0, M), slice(0, N // 64)), "rowstat")
        if self.r2 is not None:
            GR.check_canary(self.r2, (M, 2), "rowsum2")
        if f.get("slabs"):
            w = self.ws[:f["split"] * self.stride].view(f["split"], self.stride)
            win = w[:, :M * self.ld].view(f["split"], M, self.ld)
            bits = self.ws.view(torch.int32).clone()
            bw = bits[:f["split"] * self.stride].view(f["split"], self.stride)[:, :M * self.ld].view(f["split"], M, self.ld)
            bw[:, :, :N] = GR.SENTINEL_F32
            assert int((bits != GR.SENTINEL_F32).sum()) == 0, "split-K slab workspace: a write outside the slab windows"
            assert torch.isfinite(win[:, :, :N]).all()

    def check_q8(self, label, ref, rows, cols):
        """fp8 C: every sampled byte is the fp8 code of SOME value within the bound of the reference, rounded to bf16, scaled by
        FMAX / state[0] (fp32) and saturated — one code of slack only where that interval straddles a rounding midpoint; state[1] and
        the table of partial maxima as the header says"""
        from mic_amd import ops

        dt, fmax = FP8[self.c8]
        s0 = float(self.q8_state[0].item())
        scale = float(np.float32(fmax) / np.float32(s0))
        v = ref["C"]
        b = (ref["bound_C"] - GR.UBF16 * np.abs(v)) / (1 + GR.UBF16)  # the fp32 result's bound: its bf16 rounding is modelled below

        def q(x):
            t = torch.from_numpy(np.clip(x * scale, -fmax, fmax).astype(np.float32))
            return t.to(dt).float().double().numpy()

        eps = 4 * GR.U32
        lo = GR.round_bf16(v - b) - eps * np.abs(v - b)
        hi = GR.round_bf16(v + b) + eps * np.abs(v + b)
        qlo, qhi = q(lo * (1 - eps * np.sign(lo))), q(hi * (1 + eps * np.sign(hi)))
        ri, ci = torch.from_numpy(rows).to(self.dev), torch.from_numpy(cols).to(self.dev)
        got = self.C.view(torch.uint8)[:self.M, :self.N].index_select(0, ri).index_select(1, ci).view(dt).float().double().cpu().numpy()
        bad = ~((got >= qlo) & (got <= qhi))
        assert not bad.any(), f"{label} fp8 C: {int(bad.sum())} codes outside their interval, e.g. got {got[bad][:4]} lo {qlo[bad][:4]} hi {qhi[bad][:4]}"
        half = np.where(qhi > qlo, 1.0, 0.0)
        print(f"[conformance] {label} fp8 C: {got.size} codes in their intervals ({int(half.sum())} intervals straddle a midpoint)")
        assert float(self.q8_state[1].item()) == float(np.float32(s0) / np.float32(fmax)), f"{label} fp8 C: state[1]"
        P = ops.fp8_amax_partials()
        tab = self.q8_amax[:P].double().cpu().numpy()
        GR.check_canary(self.q8_amax, (slice(0, P),), "fp8 amax table")
        allq = self.C.view(torch.uint8)[:self.M, :self.N].view(dt).float().abs().max().item()
        assert (tab >= 0).all() and np.isfinite(tab).all()
        # max |bf16 result| over the whole output: within one fp8 step of the largest code (or beyond FMAX / scale when that saturates)
        lo_m = allq / scale * (1 - 2.0 ** -2)
        assert tab.max() >= lo_m and (allq >= fmax or tab.max() <= allq / scale * (1 + 2.0 ** -2)), (label, tab.max(), allq / scale)
        assert tab.max() >= (np.abs(v) - b).max()
        return 0.0

    def window_bits(self):
        out = [self.C[:self.M, :self.N].view(torch.uint8).clone() if self.c8 else self.C[:self.M, :self.N].clone()]
        if self.Z is not None:
            out.append(self.Z[:self.M, :self.N].clone())
        return out

    def check_ref(self, rng, label):
        from mic_amd import ops

        M, N, K, f, c = self.M, self.N, self.K, self.f, self.c
        rows = GR.sample_idx(M, rng)
        cols = GR.sample_idx(N, rng)
        ri, ci = torch.from_numpy(rows).to(self.dev), torch.from_numpy(cols).to(self.dev)
        kv = self.kv or K
        if c["akm"]:
            A_s = _deq(self.A[:kv].index_select(1, ri).t(), self.sa)
        else:
            A_s = _deq(self.A[:M].index_select(0, ri)[:, :K], self.sa)
        if c["bkm"]:
            B_s = _deq(self.B[:kv].index_select(1, ci), self.sb)
        else:
            B_s = _deq(self.B[:N].index_select(0, ci)[:, :K].t(), self.sb)
        A_s, B_s = A_s.cpu().numpy(), B_s.cpu().numpy()
        if not c["akm"]:
            A_s, B_s = A_s[:, :kv], B_s[:kv]

        def side(t):
            return None if t is None else t[:M, :N].index_select(0, ri).index_select(1, ci).double().cpu().numpy()

        got_C = None if self.c8 else side(self.C)
        epi = dict(alpha=f.get("alpha", 1.0), bias=None if self.bias is None else self.bias.double().cpu().numpy()[cols],
                   act=f.get("act", 0), dact=f.get("dact", 0), zin=side(self.zin), R=side(self.R), C_old=side(self.C_old),
                   c_dtype="f32" if f.get("c32") else "bf16", z_stored=side(self.Z))  # (fp8 C: bound of the bf16-rounded value)
        if f.get("drop"):
            keep = ops.dropout_mask(M * N, f["drop"], self.kw["dropout_seed"], self.dev).view(M, N)
            epi["keep"], epi["drop_p"] = side(keep), f["drop"]
        if f.get("ln"):
            st = self.ln_stats.index_select(0, ri).cpu().numpy()
            mu, rstd, d_rstd = GR.ln_fold_params(st, K, 1e-5)
            epi["ln"] = (mu, rstd, self.ln_g.double().cpu().numpy()[cols], d_rstd)
        acc = A_s @ B_s
        S = np.abs(A_s) @ np.abs(B_s)
        ref = GR.ref_epilogue(acc, S, K, **epi)
        worst = {}
        if self.Z is not None:
            worst["Z"] = GR.check(side(self.Z), ref["Z"], ref["bound_Z"], f"{label} Zout")
        if self.c8:
            worst["C8"] = self.check_q8(label, ref, rows, cols)
        else:
            worst["C"] = GR.check(got_C, ref["C"], ref["bound_C"], f"{label} C")
        if self.rs is not None:
            s, b = GR.rowsum_ref(A_s, f.get("rowsum_k", 0))
            worst["rowsum"] = GR.check(self.rs[:M].index_select(0, ri).double().cpu().numpy(), s, b, f"{label} a_rowsum")
        if self.stat is not None:
            few = ri[:8].tolist() + ri[-8:].tolist()
            Crow = self.C[:M].index_select(0, torch.tensor(few, device=self.dev))[:, :N].float().cpu().numpy()
            mx, sm = GR.rowstat_ref(Crow, f.get("nvalid", 0) or N)
            got = self.stat.index_select(0, torch.tensor(few, device=self.dev))[:, :N // 64].cpu().numpy()
            assert np.array_equal(got[..., 0], mx), f"{label} rowstat max"
            worst["rowstat"] = GR.check(got[..., 1], sm, 64 * 4 * GR.U32 * sm + 1e-30, f"{label} rowstat sum")
        if self.r2 is not None:
            Crow = self.C[:M].index_select(0, ri)[:, :N].float().cpu().numpy()
            s, b = GR.rowsum2_ref(Crow)
            worst["rowsum2"] = GR.check(self.r2[:M].index_select(0, ri).cpu().numpy().astype(np.float64), s, b, f"{label} rowsum2")
        return worst


def _launch(probs, grouped):
    from mic_amd import ops
    from mic_amd import _lib as L
    import ctypes as C

    args = [p.args() for p in probs]
    if grouped:
        ops.gemm_grouped(args)
    else:
        L.check(L.lib().mic_gemm(C.byref(args[0]), ops._stream()), "mic_gemm")
    for p in probs:
        p.finish()
    torch.cuda.synchronize()
    return args


def run_case(c, dev, *, seed=0, check_plan=True, rerun=True):
    from mic_amd import ops
    from mic_amd import _lib as L
    import ctypes as C

    gen = torch.Generator(device=dev).manual_seed(1000 + seed + sum(map(ord, c["name"])))
    rng = np.random.default_rng(seed + 7)
    probs = [Problem(c, M, N, K, f, gen, dev, i) for i, (M, N, K, f) in enumerate(GC.problems(c))]
    args = [p.args() for p in probs]
    if check_plan and c["plan"] is not None:
        arr = (L.GemmArgs * min(len(args), 8))(*args[:8])
        info = L.GemmPlanInfo()
        L.check(L.lib().mic_gemm_plan(arr, len(arr), C.byref(info)), "mic_gemm_plan")
        got = {k: getattr(info, k) for k, _ in L.GemmPlanInfo._fields_}
        switch = os.environ.get("MIC_GEMM_CONF_SWITCH")
        if switch:
            assert GC.switch_honoured(switch, c, got), (c["name"], switch, got)
        else:
            assert {k: got[k] for k in c["plan"]} == c["plan"], (c["name"], got, c["plan"])
            assert GC.kernel_name(got, c["dtype"], c["akm"], c["bkm"]) == c["kernel"], (c["name"], got)
    _launch(probs, c["group"] is not None)
    worst = {}
    for i, p in enumerate(probs):
        p.check_canaries()
        for k, v in p.check_ref(rng, f"{c['name']}[{i}]").items():
            worst[k] = max(worst.get(k, 0.0), v)
    atomic = any(p.f.get("split") and not p.f.get("slabs") for p in probs)
    if rerun and not atomic:
        first = [p.window_bits() for p in probs]
        for p in probs:
            p.outputs()
        _launch(probs, c["group"] is not None)
        for p, w in zip(probs, first):
            for a, b in zip(w, p.window_bits()):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{c['name']}: a rerun gave different bits"
            p.check_canaries()
    print(f"[conformance] {c['name']}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("name", [c["name"] for c in GC.CASES])
def test_gemm_conformance(dev, name):
    c = GC.BY_NAME[name]
    from mic_amd import ops

    try:
        if c["cus"]:
            ops.set_cu_budget(c["cus"])
        run_case(c, dev)
    finally:
        ops.set_cu_budget(0)


@pytest.mark.parametrize("cus", GC.CU_BUDGETS)
def test_gemm_conformance_cu_budget(dev, cus):
    """the persistent 256^2 grid and the K-group variants under reduced CU budgets, results checked"""
    from mic_amd import ops

    try:
        ops.set_cu_budget(cus)
        for name in GC.BUDGET_CASES:
            run_case(GC.BY_NAME[name], dev, seed=cus, check_plan=False, rerun=False)
    finally:
        ops.set_cu_budget(0)


def test_gemm_conformance_misaligned_refused_where_no_scalar_path(dev):
    """the fp8-emitting epilogue has no scalar path: a Zin / R that is not 16-B aligned is refused; so are split-K slab workspaces
    and mic_sum_slabs operands that are not 16-B aligned (both move 16-B vectors).  (The bf16 / fp32 epilogues take misaligned
    C / Z / R through their elementwise path: the misaligned_* cases.)"""
    from mic_amd import ops
    from mic_amd._lib import MicError

    M, N, K = 128, 128, 128
    a = torch.zeros(M, K, dtype=torch.float8_e4m3fn, device=dev)
    b = torch.zeros(N, K, dtype=torch.float8_e4m3fn, device=dev)
    out = torch.zeros(M, N, dtype=torch.float8_e4m3fn, device=dev)
    z = torch.zeros(M * N + 8, dtype=torch.bfloat16, device=dev)[1:1 + M * N].view(M, N)
    st = torch.ones(2, device=dev)
    with pytest.raises(MicError, match="16-B aligned"):
        ops.gemm(a, b, out, M, N, K, zin=z, dact=1, c_q8=(st, None))
    ws = torch.zeros(3 * M * N + 64, device=dev)
    with pytest.raises(MicError, match="split_stride"):
        ops.gemm(torch.zeros(M, K, dtype=torch.bfloat16, device=dev), torch.zeros(N, K, dtype=torch.bfloat16, device=dev), ws, M, N, K,
                 split_k=2, split_stride=M * N + 2)
    with pytest.raises(MicError, match="split_stride"):
        ops.gemm(torch.zeros(M, K, dtype=torch.bfloat16, device=dev), torch.zeros(N, K, dtype=torch.bfloat16, device=dev), ws[1:], M, N, K,
                 split_k=2, split_stride=M * N)
    # a slab split the reduction cannot fill (one K-tile, three slabs) is refused: it used to fill slab 0 alone (the random sweep's
    # draw 144, M = 8, N = 65, K = 64, split_k = 3, whose summed slabs came out NaN)
    with pytest.raises(MicError, match="split_k exceeds"):
        ops.gemm(torch.zeros(8, 64, dtype=torch.bfloat16, device=dev), torch.zeros(65, 64, dtype=torch.bfloat16, device=dev), ws, 8, 65, 64,
                 split_k=3, split_stride=8 * 72, ldc=72)
    # the folded LayerNorm exists on the vector epilogue only: an R or Zout that starts mid-vector is refused, not stored without it
    Kl = 256
    x = torch.zeros(M, Kl, dtype=torch.bfloat16, device=dev)
    w = torch.zeros(N, Kl, dtype=torch.bfloat16, device=dev)
    ln = dict(ln_stats=torch.zeros(M, 2, dtype=torch.int64, device=dev), ln_colsum=torch.zeros(N, device=dev), ln_width=Kl, ln_eps=1e-5,
              bias=torch.zeros(N, device=dev))
    y = torch.zeros(M, N, dtype=torch.bfloat16, device=dev)
    r = torch.zeros(M * N + 8, dtype=torch.bfloat16, device=dev)[1:1 + M * N].view(M, N)
    with pytest.raises(MicError, match="folded LayerNorm"):
        ops.gemm(x, w, y, M, N, Kl, residual=r, **ln)
    with pytest.raises(MicError, match="folded LayerNorm"):
        ops.gemm(x, w, y, M, N, Kl, zout=r, act=1, **ln)
    ops.gemm(x, w, y, M, N, Kl, residual=torch.zeros(M, N, dtype=torch.bfloat16, device=dev), **ln)  # aligned: taken
    # softmax partials are written by the bare epilogue: a group that also holds a non-PLAIN problem is refused
    st = torch.zeros(M, N // 64, 2, device=dev)
    with pytest.raises(MicError, match="rowstat"):
        ops.gemm_grouped([ops.gemm_args(x, w, y, M, N, Kl, bias=ln["bias"], rowstat=st),
                          ops.gemm_args(x, w, torch.zeros_like(y), M, N, Kl, act=2)])
    torch.cuda.synchronize()
    dst = torch.zeros(M * N + 8, device=dev)
    with pytest.raises(MicError, match="16-B aligned"):
        ops.sum_slabs(ws, 2, M * N, dst[1:], M, N, N, N)
    with pytest.raises(MicError, match="16-B aligned"):
        ops.sum_slabs(ws[1:], 2, M * N, dst, M, N, N, N)


def _random_case(i, rng):
    """one draw of the refuse-or-be-right sweep: shape, layout and feature set at random (small shapes)"""
    akm, bkm = bool(rng.integers(2)) and rng.random() < 0.3, bool(rng.integers(2))
    if akm:
        bkm = True
    M = int(rng.choice([1, 7, 8, 63, 64, 65, 120, 127, 128, 129, 191, 192, 193, 248, 255, 256, 257, 320, 500]))
    N = int(rng.choice([1, 7, 8, 56, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 384, 1000]))
    K = int(rng.choice([64, 128, 192, 320, 512, 1024])) if rng.random() < 0.95 else int(rng.choice([32, 100]))
    f = {}
    if rng.random() < 0.3:
        f["alpha"] = float(rng.choice([0.5, -2.0, 0.3125]))
    if rng.random() < 0.5:
        f["bias"] = 1
    if rng.random() < 0.4:
        f["act"] = int(rng.integers(1, 4))
        if rng.random() < 0.7:
            f["zout"] = 1
    if rng.random() < 0.25:
        f["dact"] = int(rng.integers(1, 4))
    if rng.random() < 0.25:
        f["drop"] = float(rng.choice([0.1, 0.5]))
    if rng.random() < 0.3:
        f["res"] = 1
    if rng.random() < 0.2:
        f["acc"] = 1
    if rng.random() < 0.3:
        f["c32"] = 1
    if rng.random() < 0.1:
        f["split"] = int(rng.choice([2, 3, 5]))
        if rng.random() < 0.5:
            f["slabs"] = 1
    if akm and rng.random() < 0.5:
        f["rowsum"] = 1
    if akm and bkm and rng.random() < 0.5:
        f["k_valid"] = int(rng.integers(1, K + 1))
    if rng.random() < 0.3:
        f["ldc_pad"] = int(rng.choice([0, 1, 3, 8, 13]))
    if rng.random() < 0.15:
        f["off"] = 1
    return GC.case(f"sweep{i}", M, N, K, akm=akm, bkm=bkm, **f)


def test_gemm_conformance_random_sweep(dev):
    """~200 seeded draws of shape, layout and features: every call either raises MicError or conforms"""
    from mic_amd._lib import MicError

    rng = np.random.default_rng(20261016)
    ran = refused = 0
    for i in range(200):
        c = _random_case(i, rng)
        try:
            run_case(c, dev, seed=i, check_plan=False)
            ran += 1
        except MicError:
            refused += 1
    print(f"[conformance] sweep: {ran} conformed, {refused} refused")
    assert ran >= 100


def test_gemm_conformance_behind_switches(dev):
    """the cases a latched switch can change, rerun in a child process per switch configuration — one child at a time; a child that
    fails, times out or dies on a signal ends this test at once and no further child is started.  Each child also asserts that the
    planner honours its switch on every case it runs (MIC_GEMM_CONF_SWITCH)."""
    for env, val, tag in GC.SWITCHES:
        names = [c["name"] for c in GC.CASES if tag in c["tags"]]
        assert names, tag
        kexpr = " or ".join(f"test_gemm_conformance[{n}]" for n in names)
        envd = dict(os.environ, **{env: val, "MIC_GEMM_CONF_SWITCH": f"{env}={val}"})
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                                "-k", kexpr], env=envd, capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"{env}={val}: the child timed out; no further child started\n{(e.stdout or '')[-2000:]}")
        print(f"[conformance] {env}={val}: {r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ''}")
        assert r.returncode == 0, f"{env}={val}: child rc {r.returncode}; no further child started\n" + r.stdout[-3000:] + r.stderr[-2000:]
        assert " passed" in r.stdout and "failed" not in r.stdout, r.stdout[-2000:]
