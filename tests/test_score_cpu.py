"""score(): the host-only half.  The new entry points are declared and exported, the planner gives the scorer's head launch (picked
values, no C) to gemm_d2_kernel<2> where a launch with softmax partials goes to family 6 and says so elsewhere, mic_gemm refuses the
argument sets the header names before anything is launched, the collate helpers of evaluation.py, and every refusal of `score`
before device work.  No GPU."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_SHAPE = (2432, 250112, 1024)  # the bench's LM head
KERNEL_TEST_SHAPES = [(M, Vpad, K) for M in (1, 37, 256, 300) for Vpad in (256, 1024) for K in (256, 384)]  # tests/test_head_pick_gpu.py


def test_new_entry_points_are_declared_and_exported():
    from mic_amd import _lib

    header = open(os.path.join(ROOT, "include", "mic_hip.h")).read()
    for name in ("mic_ce_rows_picked", "mic_segment_sums"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS
    assert re.search(r"const int32_t\* pick_col;\s*float\* pick_out;\s*\} mic_gemm_args;", header)  # appended: the last two fields
    assert [f[0] for f in _lib.GemmArgs._fields_][-2:] == ["pick_col", "pick_out"]


@pytest.mark.parametrize("shape", [HEAD_SHAPE] + KERNEL_TEST_SHAPES)
def test_planner_gives_pick_launches_to_d2_epi_2(shape):
    from mic_amd import ops

    plan = ops.gemm_plan([shape], kernel=True, pick=True)
    assert (plan["family"], plan["epi"], plan["tile_m"], plan["tile"]) == (6, 2, 256, 128), plan
    stat = ops.gemm_plan([shape], kernel=True, rowstat=True)  # the launch it replaces: same family, same tiling
    assert (stat["family"], stat["epi"]) == (6, 1) and stat["blocks"] == plan["blocks"], stat


@pytest.mark.parametrize("K", [64, 320])
def test_planner_says_another_family_where_d2_does_not_run(K):
    from mic_amd import ops

    plan = ops.gemm_plan([(64, 256, K)], kernel=True, pick=True)
    assert plan["family"] != 6 and plan["epi"] != 2, plan
    assert plan["family"] == ops.gemm_plan([(64, 256, K)], kernel=True, rowstat=True)["family"]


def _args(K=256, **kw):
    """a bf16 NT problem on placeholder addresses: the checks under test come before anything dereferences or launches"""
    from mic_amd import _lib as L

    g = L.GemmArgs()
    g.dtype = g.c_dtype = L.MIC_BF16
    g.M, g.N, g.K = 64, 256, K
    g.A = g.B = g.C = 4096
    g.lda = g.ldb = K
    g.ldc = 256
    for k, v in kw.items():
        setattr(g, k, v)
    return g


@pytest.mark.parametrize("kw,match", [
    (dict(pick_col=4096, pick_out=4096), "go with rowstat"),                                        # pick without rowstat
    (dict(C=None), "C may be NULL only with pick_col"),                                             # C == NULL without pick
    (dict(C=None, rowstat=4096, rowstat_ld=4), "C may be NULL only with pick_col"),                 # ... also with rowstat
    (dict(pick_col=4096, rowstat=4096, rowstat_ld=4), "both set, or neither"),                      # half a pick
    (dict(K=64, C=None, pick_col=4096, pick_out=4096, rowstat=4096, rowstat_ld=4), "family 6"),     # pick at K = 64
    (dict(K=320, pick_col=4096, pick_out=4096, rowstat=4096, rowstat_ld=4), "K=320"),               # (K % 64: the bf16 kernels' own rule)
    (dict(dtype=2, a_fmt=0, b_fmt=0, pick_col=4096, pick_out=4096, rowstat=4096, rowstat_ld=4), "bf16 operands"),  # fp8 operands
])
def test_mic_gemm_refuses_by_code_and_message(kw, match):
    from mic_amd import _lib as L

    kw = dict(kw)
    g = _args(kw.pop("K", 256), **kw)
    rc = L.lib().mic_gemm(C.byref(g), None)
    msg = L.lib().mic_last_error().decode()
    assert rc != 0 and match in msg, (rc, msg)


# ------------------------------------------------------------------------------------------------ evaluation.py helpers
def test_sequences_to_score_inputs():
    from mic_amd.evaluation import sequences_to_score_inputs

    EOS, PAD = 2, 1
    seq = np.array([[2, 9, 8, EOS, PAD, PAD],    # EOS in the middle
                    [2, 9, 8, 7, 6, EOS],        # EOS last
                    [2, 9, 8, 7, 6, 5],          # no EOS
                    [2, EOS, PAD, PAD, PAD, PAD],  # EOS at position 1
                    [2, 9, EOS, 7, EOS, PAD],    # the FIRST EOS counts
                    [2, 9, 8, PAD, PAD, PAD],    # greedy / sampled rows: the EOS that ended the row was written as PAD
                    [2, PAD, PAD, PAD, PAD, PAD]], dtype=np.int32)
    dec_in, labels, mask = sequences_to_score_inputs(seq, EOS, PAD)
    assert np.array_equal(dec_in, seq[:, :-1]) and np.array_equal(labels[:5], seq[:5, 1:])
    assert np.array_equal(labels[5:], [[9, 8, EOS, PAD, PAD], [EOS, PAD, PAD, PAD, PAD]])  # the token that was drawn there
    assert np.array_equal(mask, [[1, 1, 1, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 0, 0, 0, 0], [1, 1, 0, 0, 0],
                                 [1, 1, 1, 0, 0], [1, 0, 0, 0, 0]]) and mask.dtype == np.int32
    for bad in (seq[0], seq[:, :1], seq.astype(np.float32)):
        with pytest.raises(ValueError):
            sequences_to_score_inputs(bad, EOS, PAD)


def test_rerank_arithmetic():
    from mic_amd.evaluation import rerank, rerank_scores

    ll = np.array([-6.0, -4.0, -9.0, -1.0, -1.0, -8.0], dtype=np.float32)
    nt = np.array([3, 1, 9, 4, 2, 0], dtype=np.int32)
    best, scores = rerank_scores(ll, nt, 3, 1.0)
    assert np.allclose(scores, [[-2.0, -4.0, -1.0], [-0.25, -0.5, -np.inf]]) and best.tolist() == [2, 0] and scores.dtype == np.float32
    best, scores = rerank_scores(ll, nt, 3, 0.0)  # no length normalisation: the plain log-likelihood
    assert np.allclose(scores[0], [-6.0, -4.0, -9.0]) and best.tolist() == [1, 0]
    best, scores = rerank_scores(ll, nt, 2, 0.5)
    assert np.allclose(scores[0], [-6.0 / np.sqrt(3.0), -4.0]) and best.tolist() == [0, 1, 0]  # (-9 / 3 < -1 / 2)
    with pytest.raises(ValueError):
        rerank_scores(ll, nt, 4)

    # rerank itself: one score() call on what sequences_to_score_inputs makes of the sequences, image-major groups
    class Model:
        config = types.SimpleNamespace(mbart_config=types.SimpleNamespace(eos_token_id=2, pad_token_id=1))

        def score(self, px, labels, mask, *, decoder_input_ids, candidates_per_image):
            import torch
            assert candidates_per_image == 2 and labels.shape == (4, 3) and np.array_equal(decoder_input_ids, seq[:, :-1])
            n = mask.sum(1)
            return dict(log_likelihood=torch.tensor([-3.0, -2.0, -1.0, -4.0]), num_tokens=torch.from_numpy(n))

    seq = np.array([[2, 5, 6, 2], [2, 5, 2, 1], [2, 7, 8, 9], [2, 2, 1, 1]])
    best, scores = rerank(Model(), np.zeros((2, 4, 4, 3), np.float32), seq, 2)
    assert np.allclose(scores, [[-1.0, -1.0], [-1.0 / 3.0, -4.0]]) and best.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ score(): refusals before device work
def _stub(fp8=False):
    """what score() touches before the device: the decoder's config and the engine's GEMM mode.  Device work fails the test."""
    from mic_amd import FlaxCLIPVisionMBartForConditionalGeneration as Model

    class Stub(Model):
        def __init__(self):  # (no device, no weights)
            mc = types.SimpleNamespace(pad_token_id=1, eos_token_id=2, vocab_size=1003, max_position_embeddings=16)
            self._config = types.SimpleNamespace(mbart_config=mc)
            self.engine = types.SimpleNamespace(fp8=fp8)

        def _use_params(self, params):
            raise AssertionError("device work")

        def _dev(self, x, dtype):
            raise AssertionError("device work")
    return Stub()


PX = np.zeros((2, 4, 4, 3), np.float32)
LAB = np.array([[5, 6, 2, 1], [7, 2, 1, 1], [8, 9, 10, 2], [11, 2, 1, 1]])


@pytest.mark.parametrize("kw,match", [
    (dict(candidates_per_image=3), "2 images need 6 label rows"),
    (dict(candidates_per_image=1), "2 images need 2 label rows"),
    (dict(candidates_per_image=0), "integer >= 1"),
    (dict(candidates_per_image=2.0), "integer >= 1"),
    (dict(candidates_per_image=True), "integer >= 1"),
    (dict(labels=np.where(LAB == 9, 1003, LAB)), r"\[0, 1003\)"),
    (dict(labels=np.where(LAB == 9, -1, LAB)), r"\[0, 1003\)"),
    (dict(labels=np.where(LAB == 1, 2000, LAB), attention_mask=np.ones_like(LAB)), r"\[0, 1003\)"),
    (dict(labels=np.tile(LAB, (1, 5))), "max_position_embeddings"),
    (dict(attention_mask=np.full_like(LAB, 2)), "0/1"),
    (dict(attention_mask=np.ones((4, 3), np.int32)), "0/1"),
    (dict(decoder_input_ids=np.full_like(LAB, 1003)), "decoder_input_ids"),
    (dict(fp8=True), "fp8"),
])
def test_score_refuses_before_device_work(kw, match):
    kw = dict(kw)
    kw.setdefault("candidates_per_image", 2)
    model = _stub(kw.pop("fp8", False))
    labels = kw.pop("labels", LAB)
    with pytest.raises(ValueError, match=match):
        model.score(PX, labels, kw.pop("attention_mask", None), **kw)


def test_score_reaches_the_device_with_valid_arguments():
    out_of_range_behind_the_mask = np.where(LAB == 1, 5000, LAB)  # ids on masked positions are not looked at
    for labels, mask in ((LAB, None), (out_of_range_behind_the_mask, (LAB != 1).astype(np.int64))):
        with pytest.raises(AssertionError, match="device work"):
            _stub().score(PX, labels, mask, candidates_per_image=2)
