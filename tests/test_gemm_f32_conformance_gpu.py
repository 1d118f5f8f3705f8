"""fp32 GEMM conformance on the MI355X: every case of tests/util_gemm_f32_cases.py — gemm_f32_kernel (the parity mode every fp32
claim of the suite rests on) through the scalar epilogue epilogue_store<float>, and act_fwd / act_bwd at fp32 resolution through
the fp32 kernel and through the bf16 kernels' vector epilogue — element-wise against the fp64 reference of tests/util_gemm_ref.py.
Around every call:
  - the operands lie in NaN-padded allocations with odd leading dimensions and must hold the same bits afterwards;
  - C and Zout lie in canary-filled allocations, one element past a 16-byte boundary, with ldc != ldz != ldr; every element outside
    the output windows, before and behind the offset views included, must keep its bits;
  - a second launch gives identical bits (no atomics on this path).
Further: position independence of the k order (a sub-problem equals that window of the full result bit for bit), a report of how
many elements differ from a numpy fp32 multiply-add chain (no assertion), and every argument set the header says the f32 path
refuses (MIC_EINVAL, mic_last_error set, nothing written)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_gemm_f32_cases as FC  # noqa: E402
import util_gemm_ref as GR  # noqa: E402

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).clone()


class Offset:
    """a [rows][ld] view that starts `off` elements into a flat allocation: canary-filled (an output) or holding `init` (an input)"""

    def __init__(self, rows, ld, dtype, dev, off, init=None):
        n = rows * ld
        self.flat = torch.empty(n + 16, dtype=dtype, device=dev)
        self.off, self.n = off, n
        self.view = self.flat[off:off + n].view(rows, ld)
        if init is None:
            GR.sentinel_fill(self.flat)
        else:
            self.flat.fill_(float("nan"))
            self.view.copy_(torch.from_numpy(init).to(dev))

    def check_canary(self, M, N, what):
        GR.check_canary(self.view, (M, N), what)
        GR.check_canary(self.flat[:self.off], None, what + " (before the view)")
        GR.check_canary(self.flat[self.off + self.n:], None, what + " (behind the view)")


class Problem:
    """one materialised problem on the device"""

    def __init__(self, h, dev):
        self.h, self.dev = h, dev
        self.dt = torch.bfloat16 if h["dtype"] == "bf16" else torch.float32
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev).to(self.dt)  # noqa: E731
        self.A, self.B = up(h["A"]), up(h["B"])
        self.bias = None if h["bias"] is None else torch.from_numpy(h["bias"]).to(dev)
        M = h["M"]
        self.Zin = None if h["Zin"] is None else Offset(M + 2, h["ldz"], self.dt, dev, h["off"], h["Zin"])
        self.R = None if h["R"] is None else Offset(M + 2, h["ldr"], self.dt, dev, h["off"], h["R"])
        self.inputs = [t for t in (self.A, self.B, self.bias, self.Zin and self.Zin.flat, self.R and self.R.flat) if t is not None]
        self.before = [_bits(t) for t in self.inputs]
        self.outputs()

    def outputs(self):
        h = self.h
        M, N = h["M"], h["N"]
        self.C = Offset(M + 2, h["ldc"], torch.float32, self.dev, h["off"])
        if h["C_old"] is not None:
            self.C.view[:M, :N] = torch.from_numpy(h["C_old"]).to(self.dev)
        self.Z = Offset(M + 2, h["ldz"], self.dt, self.dev, h["off"]) if h["f"].get("zout") else None

    def args(self):
        from mic_amd import ops

        h, f = self.h, self.h["f"]
        return ops.gemm_args(self.A, self.B, self.C.view, h["M"], h["N"], h["K"], a_kmajor=h["akm"], b_kmajor=h["bkm"], bias=self.bias,
                             act=f.get("act", 0), zout=self.Z and self.Z.view, zin=self.Zin and self.Zin.view, dact=f.get("dact", 0),
                             residual=self.R and self.R.view, accumulate=bool(f.get("acc")), dropout_p=f.get("drop", 0.0),
                             dropout_seed=h["seed"] & 0xFFFFFFFF, alpha=f.get("alpha", 1.0), lda=h["lda"], ldb=h["ldb"], ldc=h["ldc"],
                             ldz=h["ldz"], ldr=h["ldr"])

    def windows(self):
        M, N = self.h["M"], self.h["N"]
        c = self.C.view[:M, :N].cpu().numpy()
        z = None if self.Z is None else self.Z.view[:M, :N].float().cpu().numpy()
        return c, z

    def check_untouched(self, label):
        M, N = self.h["M"], self.h["N"]
        self.C.check_canary(M, N, f"{label} C")
        if self.Z is not None:
            self.Z.check_canary(M, N, f"{label} Zout")
        for t, b in zip(self.inputs, self.before):
            assert torch.equal(_bits(t), b), f"{label}: an input buffer changed"


def _launch(probs, grouped):
    from mic_amd import _lib as L
    from mic_amd import ops

    args = [p.args() for p in probs]
    if grouped:
        ops.gemm_grouped(args)
    else:
        for a in args:
            L.check(L.lib().mic_gemm(C.byref(a), ops._stream()), "mic_gemm")
    torch.cuda.synchronize()


_RESULTS = {}  # case name -> [(h, C window)]: the position-independence test and the fma-chain report reuse the layout results


def run_case(c, dev):
    probs = [Problem(FC.materialise(p, FC.seed_of(c["name"], i)), dev) for i, p in enumerate(c["probs"])]
    _launch(probs, c["grouped"])
    worst, first = {}, []
    for i, p in enumerate(probs):
        label = f"{c['name']}[{i}]"
        p.check_untouched(label)
        cw, zw = p.windows()
        first.append((cw, zw))
        A, B = FC.windows(p.h)
        for k, v in GR.check_problem(p.h, A, B, cw, zw, label).items():
            worst[k] = max(worst.get(k, 0.0), v)
    for p in probs:
        p.outputs()
    _launch(probs, c["grouped"])
    for i, (p, (cw, zw)) in enumerate(zip(probs, first)):
        p.check_untouched(f"{c['name']}[{i}] (second launch)")
        c2, z2 = p.windows()
        assert GR.same_bits(cw, c2) and (zw is None or GR.same_bits(zw, z2)), f"{c['name']}[{i}]: a second launch gave different bits"
    _RESULTS[c["name"]] = [(p.h, cw) for p, (cw, _) in zip(probs, first)]
    print(f"[f32 conformance] {c['family']} {c['name']}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return probs


@pytest.mark.parametrize("name", [c["name"] for c in FC.CASES])
def test_gemm_f32_conformance(dev, name):
    run_case(FC.BY_NAME[name], dev)


@pytest.mark.parametrize("tag", [t for t, _, _ in FC.LAYOUTS])
def test_position_independence(dev, tag):
    """rows [64, 129) x columns [64, 127) of the (129, 127, 200) problem, launched as a problem of their own on the same operands:
    every output element sees the same k order wherever it sits in a tile, so the bits equal that window of the full result"""
    from mic_amd import _lib as L
    from mic_amd import ops

    M, N, K = FC.WINDOW_CASE
    r0, c0 = FC.WINDOW_AT
    c = FC.BY_NAME[f"layout_{M}x{N}x{K}_{tag}"]
    p = run_case(c, dev)[0]
    full, _ = p.windows()
    h = p.h
    a = p.A[:, r0:] if h["akm"] else p.A[r0:]
    b = p.B[:, c0:] if h["bkm"] else p.B[c0:]
    Ms, Ns = M - r0, N - c0
    out = Offset(Ms + 2, Ns + 5, torch.float32, dev, 1)
    g = ops.gemm_args(a, b, out.view, Ms, Ns, K, a_kmajor=h["akm"], b_kmajor=h["bkm"], lda=h["lda"], ldb=h["ldb"], ldc=Ns + 5)
    L.check(L.lib().mic_gemm(C.byref(g), ops._stream()), "mic_gemm")
    torch.cuda.synchronize()
    out.check_canary(Ms, Ns, "window C")
    assert GR.same_bits(out.view[:Ms, :Ns].cpu().numpy(), full[r0:, c0:]), "the window of the full result differs from the sub-problem"


def test_report_fma_chain(dev):
    """report only: over the layout cases, how many output elements differ from the numpy fp32 chain (k ascending, one rounding per
    multiply-add: util_gemm_ref.emu_gemm) — the header calls the kernel a bit-exact fp32 fma chain"""
    differ = total = 0
    worst_ulp = 0.0
    for c in FC.CASES:
        if c["family"] != "layouts":
            continue
        if c["name"] not in _RESULTS:
            run_case(c, dev)
        for h, cw in _RESULTS[c["name"]]:
            emu = GR.emu_gemm(h)["C"][:h["M"], :h["N"]]
            ne = emu.view(np.uint32) != np.ascontiguousarray(cw).view(np.uint32)
            differ += int(ne.sum())
            total += ne.size
            if ne.any():
                worst_ulp = max(worst_ulp, float((np.abs(emu.astype(np.float64) - cw)[ne] / np.spacing(np.abs(emu[ne]))).max()))
    print(f"[f32 conformance] fma chain: {differ} of {total} layout outputs differ from the numpy fp32 chain (largest difference {worst_ulp:.3g} ulp)")


def _refusal_base(dev):
    """a small valid fp32 problem with every output in canary allocations, and canary buffers for the by-products it must not get"""
    h = FC.materialise(FC.prob(5, 6, 7), 1)
    p = Problem(h, dev)
    extra = {k: GR.sentinel_fill(torch.empty(64, dtype=dt, device=dev)) for k, dt in
             (("a_rowsum", torch.float32), ("rowstat", torch.float32), ("rowsum2", torch.int64), ("ln_stats", torch.int64),
              ("ln_colsum", torch.float32), ("zout", torch.float32))}
    return p, extra


def _set(**kw):
    def f(g, x):
        for k, v in kw.items():
            setattr(g, k, v(x) if callable(v) else v)
    return f


REFUSALS = [
    ("split_k=2", _set(split_k=2)),
    ("a_rowsum", _set(a_rowsum=lambda x: x["a_rowsum"].data_ptr())),
    ("k_valid", _set(k_valid=4)),
    ("rowstat", _set(rowstat=lambda x: x["rowstat"].data_ptr(), rowstat_ld=1)),
    ("a_ln_stats", _set(a_ln_stats=lambda x: x["ln_stats"].data_ptr(), a_ln_colsum=lambda x: x["ln_colsum"].data_ptr(), a_ln_width=7,
                        a_ln_eps=1e-5, bias=lambda x: x["ln_colsum"].data_ptr())),
    ("rowsum2", _set(rowsum2=lambda x: x["rowsum2"].data_ptr())),
    ("c_dtype=bf16", _set(c_dtype=0)),
    ("c_dtype=fp8", _set(c_dtype=2)),
    ("dact without Zin", _set(dact=1, Zin=None)),
    ("dropout_p=1.0", _set(dropout_p=1.0)),
    ("dropout_p=-0.1", _set(dropout_p=-0.1)),
    ("M=0", _set(M=0)), ("N=0", _set(N=0)), ("K=0", _set(K=0)),
    ("A=NULL", _set(A=None)), ("B=NULL", _set(B=None)), ("C=NULL", _set(C=None)),
]


@pytest.mark.parametrize("what", [w for w, _ in REFUSALS])
def test_refused(dev, what):
    """what the header says the f32 path refuses (and what mic_gemm refuses for every dtype) returns MIC_EINVAL with a message and
    writes nothing — not a feature silently ignored"""
    from mic_amd import _lib as L
    from mic_amd import ops

    assert (L.MIC_BF16, L.MIC_F32, L.MIC_FP8) == (0, 1, 2)
    p, extra = _refusal_base(dev)
    g = p.args()
    g.Zout, g.ldz = extra["zout"].data_ptr(), 8  # an output the refused call must leave alone as well
    dict(REFUSALS)[what](g, extra)
    rc = L.lib().mic_gemm(C.byref(g), ops._stream())
    msg = L.lib().mic_last_error().decode()
    torch.cuda.synchronize()
    assert rc == -1, (what, rc, msg)  # MIC_EINVAL
    assert msg.startswith("mic_gemm"), (what, msg)
    p.check_untouched(what)
    GR.check_canary(p.C.flat, None, f"{what}: C")
    for k, t in extra.items():
        GR.check_canary(t, None, f"{what}: {k}")
    # ... and through the grouped entry point, which runs fp32 problems one by one
    rc = L.lib().mic_gemm_grouped((L.GemmArgs * 1)(g), 1, ops._stream())
    torch.cuda.synchronize()
    assert rc == -1 and L.lib().mic_last_error().decode().startswith("mic_gemm"), (what, rc)
    GR.check_canary(p.C.flat, None, f"{what}: C (grouped)")
