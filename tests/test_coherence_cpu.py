"""The weight-coherence checkers without a GPU: every comparison core of tests/util_coherence.py accepts a clean copy and rejects a
planted defect, and the event x mode table of the device sweep is complete.  The "device results" here come from the references the
cores compare against (util_gemm_ref.round_bf16, util_rowop_ref.fold_ref / emu_transpose, util_fp8_ref.emit_ref), applied to the right
or to the wrong source."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_coherence as C  # noqa: E402
import util_fp8_ref as F8  # noqa: E402
import util_rowop_ref as RR  # noqa: E402
from util_gemm_ref import round_bf16  # noqa: E402

F = np.float32


def _bf16(rng, *shape, scale=1.0):
    return round_bf16(scale * rng.standard_normal(shape)).astype(F)


# ------------------------------------------------------------------------------------------------ lp
def test_lp_core_accepts_the_rounded_master_and_rejects_one_stale_element():
    rng = np.random.default_rng(1)
    old = (0.02 * rng.standard_normal(4096)).astype(F)
    new = old.copy()
    new[1234] += F(1e-3)  # one optimizer update
    lp = C.bf16_bits(round_bf16(new))
    C.core_lp(lp, new)
    stale = lp.copy()
    stale[1234] = C.bf16_bits(round_bf16(old))[1234]
    assert stale[1234] != lp[1234]
    with pytest.raises(AssertionError, match="1 of 4096"):
        C.core_lp(stale, new)


def test_lp_core_rejects_truncation_on_a_tie():
    """1 + 2^-8 lies halfway between the bf16 neighbours 1 and 1 + 2^-7: round-to-nearest-even gives 1 (even mantissa), and
    1 + 3 * 2^-8 gives 1 + 2^-6 where truncation gives 1 + 2^-7"""
    master = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 3 * 2.0 ** -8, 0.5], dtype=F)
    rne = C.bf16_bits(round_bf16(master))
    trunc = (master.view(np.uint32) >> 16).astype(np.uint16)
    assert rne[0] == trunc[0] == 0x3F80 and rne[1] == 0x3F82 and trunc[1] == 0x3F81 and rne[3] == trunc[3]
    C.core_lp(rne, master)
    with pytest.raises(AssertionError, match="2 of 4"):
        C.core_lp(trunc, master)


# ------------------------------------------------------------------------------------------------ E^T
def test_transposed_core_accepts_the_transpose_and_rejects_the_previous_weights():
    rng = np.random.default_rng(2)
    E_old = C.bf16_bits(_bf16(rng, 256, 128, scale=0.02))
    E_new = E_old.copy()
    E_new[17, 5] ^= 0x0001  # the last mantissa bit of one element moved
    C.core_transposed(RR.emu_transpose(E_new, 256, 256), E_new)
    with pytest.raises(AssertionError, match="transpose"):
        C.core_transposed(RR.emu_transpose(E_old, 256, 256), E_new)
    with pytest.raises(AssertionError, match="shape"):
        C.core_transposed(RR.emu_transpose(E_new, 256, 256)[:, :128], E_new)


# ------------------------------------------------------------------------------------------------ LayerNorm folds
def _fold(w, gamma, beta, bias):
    wf, cs, _, bf, _ = RR.fold_ref(w, gamma, beta, bias, "bf16")
    return C.bf16_bits(wf), cs.astype(F), bf.astype(F)


def test_fold_core_accepts_the_fold_and_rejects_the_old_gamma_beta_and_weight():
    rng = np.random.default_rng(3)
    N, K = 96, 128
    w = _bf16(rng, N, K, scale=0.05)
    gamma, beta, bias = (1.0 + 0.2 * rng.standard_normal(K)).astype(F), (0.2 * rng.standard_normal(K)).astype(F), rng.standard_normal(N).astype(F)
    good = _fold(w, gamma, beta, bias)
    C.core_fold(good, w, gamma, beta, bias, "clean", fresh=good)
    g2 = gamma.copy()
    g2[7] *= F(1.5)
    with pytest.raises(AssertionError, match="w_fold"):
        C.core_fold(_fold(w, gamma, beta, bias), w, g2, beta, bias, "old gamma")
    b2 = beta + F(0.05)
    with pytest.raises(AssertionError, match="bias'"):
        C.core_fold(_fold(w, gamma, beta, bias), w, gamma, b2, bias, "old beta")
    w2 = w.copy()
    w2[3] = round_bf16(w2[3] * 1.25).astype(F)
    with pytest.raises(AssertionError, match="w_fold"):
        C.core_fold(_fold(w, gamma, beta, bias), w2, gamma, beta, bias, "old weight")
    with pytest.raises(AssertionError, match="fresh fold"):
        C.core_fold(good, w, gamma, beta, bias, "fresh differs", fresh=_fold(w, g2, beta, bias))


# ------------------------------------------------------------------------------------------------ shortlist
def test_gather_core_accepts_the_gather_and_rejects_old_rows_old_bias_and_dirty_padding():
    rng = np.random.default_rng(4)
    V, d = 300, 64
    shared, flb = C.bf16_bits(_bf16(rng, V, d)), rng.standard_normal(V).astype(F).view(np.uint32)
    ids = np.sort(rng.choice(V, 41, replace=False)).astype(np.int32)
    E, b = np.zeros((128, d), np.uint16), np.zeros(128, np.uint32)
    E[:41], b[:41] = shared[ids], flb[ids]
    C.core_gather(E, b, shared, flb, ids)
    s2 = shared.copy()
    s2[ids[40], 3] ^= 1
    with pytest.raises(AssertionError, match="gathered rows"):
        C.core_gather(E, b, s2, flb, ids)
    f2 = flb.copy()
    f2[ids[0]] ^= 1
    with pytest.raises(AssertionError, match="gathered bias"):
        C.core_gather(E, b, shared, f2, ids)
    E2 = E.copy()
    E2[100, 0] = 1
    with pytest.raises(AssertionError, match="padding"):
        C.core_gather(E2, b, shared, flb, ids)


# ------------------------------------------------------------------------------------------------ fp8 weight copies
def _q8(src, amax_old):
    b, sinv, amax = F8.emit_ref(src, amax_old, "e4m3")
    return dict(q=b, qT=np.ascontiguousarray(b.T), state=np.array([amax if amax_old is None else amax_old, sinv], dtype=F))


def test_fp8_core_accepts_both_scale_sources_and_rejects_the_wrong_amax_and_a_qT_that_is_not_the_transpose():
    rng = np.random.default_rng(5)
    src = _bf16(rng, 64, 128, scale=0.05)
    prev = round_bf16(src * 1.01 + 0.001).astype(F)  # the weights one optimizer step earlier
    a_prev, a_now = float(np.abs(prev).max()), float(np.abs(src).max())
    assert a_prev != a_now
    C.core_fp8(_q8(src, None), src, None, "current amax")
    C.core_fp8(_q8(src, a_prev), src, a_prev, "the previous step's amax")
    with pytest.raises(AssertionError):  # bytes quantised under the wrong amax: the history was not restarted
        C.core_fp8(_q8(src, a_prev), src, None, "wrong amax")
    with pytest.raises(AssertionError):  # ... or restarted where it should have rolled
        C.core_fp8(_q8(src, None), src, a_prev, "wrong amax")
    with pytest.raises(AssertionError):  # the copy of the previous weights
        C.core_fp8(_q8(prev, None), src, None, "old weights")
    got = _q8(src, None)
    got["qT"] = got["qT"].copy()
    got["qT"][5, 9] ^= 0x01
    with pytest.raises(AssertionError):
        C.core_fp8(got, src, None, "qT")
    # a qT that differs from q.T only in the sign of a zero passes the byte reference (both zeros count) but not the transpose check
    z = src.copy()
    z[2, 3] = 0.0
    got = _q8(z, None)
    assert got["q"][2, 3] == 0
    got["qT"] = got["qT"].copy()
    got["qT"][3, 2] = 0x80
    with pytest.raises(AssertionError, match="qT against q.T"):
        C.core_fp8(got, z, None, "qT zero sign")


# ------------------------------------------------------------------------------------------------ params cache
def test_params_core_accepts_equal_leaves_and_rejects_a_stale_or_missing_leaf():
    rng = np.random.default_rng(6)
    exp = {"a/kernel": rng.standard_normal((4, 5)).astype(F), "a/bias": rng.standard_normal(5).astype(F)}
    C.core_params({k: v.copy() for k, v in exp.items()}, exp)
    stale = {k: v.copy() for k, v in exp.items()}
    stale["a/bias"][2] += F(1e-3)
    with pytest.raises(AssertionError, match="a/bias"):
        C.core_params(stale, exp)
    with pytest.raises(AssertionError, match="leaf names"):
        C.core_params({"a/kernel": exp["a/kernel"]}, exp)


# ------------------------------------------------------------------------------------------------ the sweep is complete
EXPECTED_EVENTS = {  # the ways the weights move, and the modes each applies to (the Trainer refuses E3 - E5 beside fp8 GEMMs)
    "E1_step": C.ALL, "E2_step_one_launch": C.ALL, "E3_accumulate": C.NO_FP8, "E4_clip": C.NO_FP8, "E5_groups": C.NO_FP8,
    "E6_setter": C.ALL, "E7_restore": C.ALL, "E8_raised": C.ALL, "E9_step_restore": C.ALL, "E9_setter_step": C.ALL}


def test_the_event_by_mode_table_is_complete():
    assert tuple(C.MODES) == ("fp32", "bf16", "bf16wide", "fp8delayed", "fp8current") == C.ALL and C.NO_FP8 == C.ALL[:3]
    assert set(C.EVENTS) == set(EXPECTED_EVENTS) == set(C.DRIVERS)
    for e, modes in EXPECTED_EVENTS.items():
        assert C.EVENTS[e]["modes"] == modes, e
        for m in modes:
            assert (m, e) in C.MATRIX, (m, e)
    assert len(C.MATRIX) == len(set(C.MATRIX)) == sum(len(m) for m in EXPECTED_EVENTS.values()) == 7 * 5 + 3 * 3
    # every row of the inventory has a checker and exists in some mode; every mode names rows of the inventory only
    assert tuple(C.CHECKERS) == C.INVENTORY
    assert set().union(*(set(md["rows"]) for md in C.MODES.values())) == set(C.INVENTORY)
    assert all(set(md["rows"]) <= set(C.INVENTORY) and {"lp", "shortlist", "params"} <= set(md["rows"]) for md in C.MODES.values())
    assert "shared_T" in C.MODES["bf16wide"]["rows"] and all("fp8" in C.MODES[m]["rows"] for m in ("fp8delayed", "fp8current"))
    assert all("ln_folds" in md["rows"] for m, md in C.MODES.items() if m != "fp32")


def test_the_sweep_of_the_device_suite_is_the_table():
    """tests/test_coherence_gpu.py parametrises both sweeps over MATRIX itself (read from its source: importing it needs no GPU, but
    the claim is about what is written there)"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_coherence_gpu.py")).read()
    assert src.count('@pytest.mark.parametrize("mode,event", C.MATRIX, ids=IDS)') == 2
    assert "mark.skip" not in src and "pytest.skip" not in src and "xfail" not in src


def test_the_trainer_refuses_what_the_table_leaves_out():
    """E3 - E5 are absent for the fp8 modes because the Trainer refuses the combination, not because the sweep forgot them"""
    from mic_amd.train import _check_param_groups  # noqa: F401  (the module imports without a GPU)
    import inspect

    from mic_amd import train

    text = inspect.getsource(train.Trainer.__init__)
    for what in ("param_groups is not supported together with gemm_dtype='fp8'", "max_grad_norm is not supported together with gemm_dtype='fp8'",
                 "accumulate_steps > 1 is not supported together with gemm_dtype='fp8'"):
        assert what in text, what


def test_the_wide_vocabulary_reaches_the_nt_head_backward_and_the_fp8_widths_the_fp8_head():
    """host arithmetic of Engine._head_nt_kcap and Fp8State.head on the reduced configurations"""
    from util_small import SMALL

    d = SMALL["d_model"]
    vpad = (C.WIDE_VOCAB + 127) // 128 * 128
    assert C.WIDE_VOCAB > 16384 and vpad >= 16384 and d % 128 == 0 and vpad * 128 * 2 < 0x7fffffff
    assert (SMALL["vocab_size"] + 127) // 128 * 128 < 16384  # the plain reduced models do not build E^T
    assert C.FP8_WIDTHS["d_model"] % 128 == 0 and C.FP8_WIDTHS["d_model"] // C.FP8_WIDTHS["d_heads"] == 64
    assert 2 in C.ALLOWED and len(C.ALLOWED) >= 2 * C.GEN_BEAM["num_beams"] and C.ALLOWED.max() < SMALL["vocab_size"]
