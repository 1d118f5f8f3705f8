"""The fp32 GEMM conformance suite's own checks, on a machine without a GPU.  `emu_gemm` (tests/util_gemm_ref.py) restates the
contract of gemm_f32_kernel + epilogue_store in numpy fp32: it reads the NaN-padded operand allocations through lda / ldb, steps k by
16 in ascending order with one rounding per multiply-add, and runs the header's epilogue order on the formulas of csrc/common.h.
  - without a defect it passes every case of tests/util_gemm_f32_cases.py, the activation sweeps included, with worst
    err / bound <= 1: the bounds the GPU module asserts are reachable by a correct implementation;
  - each listed defect is rejected on a named case, by the same comparison (`check_problem`) and canary check the GPU module runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_gemm_f32_cases as FC  # noqa: E402
import util_gemm_ref as GR  # noqa: E402


def run_emulated(c, defect=None, log=False):
    """every problem of a case through the emulation and the GPU module's checks; {'C': worst err / bound, 'Z': ...}"""
    worst = {}
    for i, p in enumerate(c["probs"]):
        h = FC.materialise(p, FC.seed_of(c["name"], i))
        out = GR.emu_gemm(h, defect)
        M, N = h["M"], h["N"]
        assert GR.canary_intact(out["C"], M, N), f"{c['name']}[{i}]: C written outside its window"
        assert out["Z"] is None or GR.canary_intact(out["Z"], M, N), f"{c['name']}[{i}]: Zout written outside its window"
        A, B = FC.windows(h)
        Z = None if out["Z"] is None else out["Z"][:M, :N]
        for k, v in GR.check_problem(h, A, B, out["C"][:M, :N], Z, f"{c['name']}[{i}]", log=log).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.parametrize("family", FC.FAMILIES)
def test_emulation_conforms(family):
    """the defect-free emulation passes every case of the family; the worst err / bound is printed"""
    worst = {}
    for c in FC.CASES:
        if c["family"] == family:
            for k, v in run_emulated(c).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"[f32 conformance] emulation, {family}: worst err/bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert worst and max(worst.values()) <= 1.0


# defect -> a case that must reject it
REJECTED_ON = [
    ("k_tail_dropped", "layout_31x33x15_nn"),
    ("k_tail_dropped", "layout_129x127x200_tt"),
    ("col_past_k", "layout_32x32x17_nn"),
    ("col_past_k", "layout_65x63x33_tn"),
    ("row_past_m", "layout_63x65x16_nn"),
    ("row_past_m", "layout_65x63x33_tt"),
    ("ldz_for_r", "epi_65x67x40_res"),
    ("drop_idx_ldc", "epi_65x67x40_drop05"),
    ("drop_idx_ldc", "epi_96x72x48_drop01"),
    ("alpha_after_bias", "epi_96x72x48_fwd_chain"),
    ("bias_after_act", "epi_65x67x40_fwd_chain"),
    ("act_unrounded", "sweep_bf16_fwd_act1_alpha"),
    ("act_unrounded", "sweep_bf16_fwd_act2_alpha"),
    ("act_unrounded", "sweep_bf16_fwd_act3_alpha"),
    ("acc_ignored", "epi_96x72x48_acc"),
    ("acc_ignored", "epi_65x67x40_bwd_chain"),
    ("dact_wrong_id", "epi_96x72x48_dact1"),
    ("dact_wrong_id", "sweep_f32_bwd_act1"),
    ("dact_wrong_id", "sweep_bf16_bwd_act1"),
    ("sam_sak_swapped", "layout_31x33x15_tn"),
    ("sam_sak_swapped", "layout_64x64x64_tt"),
    ("gelu_tanh_nan", "sweep_f32_fwd_act2"),
    ("gelu_tanh_nan", "sweep_bf16_fwd_act2"),
]


def test_every_listed_defect_is_exercised():
    assert {d for d, _ in REJECTED_ON} == set(GR.DEFECTS)


@pytest.mark.parametrize("defect,name", REJECTED_ON)
def test_defect_is_rejected(defect, name):
    c = FC.BY_NAME[name]
    run_emulated(c)  # the case itself conforms ...
    with pytest.raises(AssertionError):  # ... and the defect does not
        run_emulated(c, defect)


def test_unrounded_act_cannot_show_on_the_bf16_grid():
    """why the table carries the alpha = 1 + 2^-9 variants: on the plain bf16 grid every pre-activation is a bf16 number"""
    run_emulated(FC.BY_NAME["sweep_bf16_fwd_act1"], "act_unrounded")


def test_table_keeps_its_conventions():
    names = [c["name"] for c in FC.CASES]
    assert len(names) == len(set(names))
    assert sum(c["family"] == "layouts" for c in FC.CASES) == 4 * len(FC.LAYOUT_SHAPES) == 40
    assert sum(c["family"] == "epilogue" for c in FC.CASES) == 2 * 19
    assert len(FC.BY_NAME["grouped_eleven_f32"]["probs"]) == 11
    for c in FC.CASES:
        for i, p in enumerate(c["probs"]):
            h = FC.materialise(p, FC.seed_of(c["name"], i))
            M, N, K = h["M"], h["N"], h["K"]
            A, B = FC.windows(h)
            for t, win in ((h["A"], A), (h["B"], B)):
                assert np.isnan(t).sum() == t.size - win.size  # NaN everywhere outside the window, nowhere inside
                nz = np.abs(win[win != 0])
                assert nz.size == 0 or nz.min() >= np.finfo(np.float32).tiny  # normal numbers or exact zeros
            if p["dtype"] == "f32":
                ext_a, ext_b = (M if h["akm"] else K), (N if h["bkm"] else K)
                assert (h["lda"], h["ldb"], h["ldc"], h["ldz"], h["ldr"], h["off"]) == (ext_a + 3, ext_b + 3, N + 5, N + 1, N + 9, 1)
                assert h["A"].shape[0] == (K if h["akm"] else M) + 2 and h["B"].shape[0] == (K if h["bkm"] else N) + 2
            else:
                assert h["lda"] % 8 == 0 and h["ldb"] % 8 == 0 and h["ldc"] % 8 == 0 and h["ldz"] % 8 == 0 and K % 64 == 0
                assert GR.same_bits(GR.round_bf16(A), A) and GR.same_bits(GR.round_bf16(B), B)
            if p["f"].get("sweep"):
                g = np.abs(h["grid"][h["grid"] != 0])
                assert g.min() == 2.0 ** -24 and g.max() < 512 and (h["grid"][-1] == 0).all()
                assert np.array_equal(GR.round_to(h["grid"], "bf16" if p["dtype"] == "bf16" else "f32"), h["grid"])  # exact products
