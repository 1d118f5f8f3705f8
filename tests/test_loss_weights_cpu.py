"""Per-caption loss weights on the host: the weighted restatement of the oracle's loss, the self-critical helpers and their sign, the
refusals of batch["loss_weights"] before anything touches a device, the header, and the fixture of tests/test_loss_weights_gpu.py.  No
GPU needed."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import util_loss_weights_ref as LW  # noqa: E402
from test_captions_per_image_cpu import _batch, _trainer  # noqa: E402


# ------------------------------------------------------------------------------------------------ the restated loss
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_weights_of_one_give_the_oracles_loss_bitwise(ls):
    from oracle import train_ref

    g = torch.Generator().manual_seed(5)
    B, T, V = 6, 12, 1003
    logits = torch.randn(B, T, V, generator=g) * 3
    labels = torch.randint(0, V, (B, T), generator=g)
    mask = (torch.arange(T)[None] < torch.randint(2, T, (B, 1), generator=g)).to(torch.int64)
    ref = train_ref.loss_fn(logits, labels, mask, ls)
    for w in (torch.ones(B), torch.ones(B, T)):
        got = LW.weighted_loss_fn(logits, labels, mask, w, ls)
        assert got.numpy().tobytes() == ref.numpy().tobytes(), (ls, tuple(w.shape), got.item(), ref.item())
    # and the weights do something: the definition, in fp64
    w = torch.tensor(LW.WEIGHTS)
    got = LW.weighted_loss_fn(logits, labels, mask, w, ls).item()
    per = torch.stack([train_ref.loss_fn(logits[b:b + 1], labels[b:b + 1], mask[b:b + 1], ls) * mask[b].sum() for b in range(B)]).double()
    want = float((per * w.double()).sum() / mask.sum())
    assert abs(got - want) < 1e-5 * max(1.0, abs(want)) and abs(got - ref.item()) > 1e-3


# ------------------------------------------------------------------------------------------------ self-critical helpers
def test_scst_advantages_arithmetic():
    from mic_amd.evaluation import scst_advantages

    r = np.array([1.0, 2.0, 6.0, 0.5, 0.5, 0.5])
    a = scst_advantages(r, 3)
    assert a.dtype == np.float32 and a.shape == (6,)
    assert np.allclose(a, [1 - 4, 2 - 3.5, 6 - 1.5, 0, 0, 0])
    assert np.array_equal(a, scst_advantages(r, 3, baseline="mean_others"))
    m = scst_advantages(r, 3, baseline="mean")
    assert np.allclose(m, [-2, -1, 3, 0, 0, 0]) and abs(m[:3].sum()) < 1e-6
    # mean_others is the mean baseline scaled by n / (n - 1)
    assert np.allclose(a, m * 3 / 2)
    e = scst_advantages(r, 3, baseline=np.array([2.0, 1.0]))
    assert np.allclose(e, [-1, 0, 4, -0.5, -0.5, -0.5])
    assert np.allclose(scst_advantages([3.0, 5.0], 1, baseline="mean"), [0, 0])
    assert np.allclose(scst_advantages([3.0, 5.0], 1, baseline=[1.0, 1.0]), [2, 4])
    with pytest.raises(ValueError, match="mean_others"):
        scst_advantages([3.0, 5.0], 1)
    for bad in (dict(n_per_image=4), dict(n_per_image=0), dict(n_per_image=3, baseline="median"), dict(n_per_image=3, baseline=np.zeros(3))):
        with pytest.raises(ValueError):
            scst_advantages(r, **bad)


class _GenStub:
    """a model that `generates` fixed rows: two images, three samples each, start token 2 first, EOS 2 / PAD 1 behind the captions"""
    config = types.SimpleNamespace(mbart_config=types.SimpleNamespace(eos_token_id=2, pad_token_id=1))
    SEQ = np.array([[2, 7, 7, 7, 2, 1], [2, 7, 9, 2, 1, 1], [2, 9, 9, 9, 9, 2],
                    [2, 5, 2, 1, 1, 1], [2, 7, 5, 5, 2, 1], [2, 5, 5, 7, 7, 2]], np.int32)

    def generate(self, pixel_values, **kw):
        self.kw = kw
        return types.SimpleNamespace(sequences=torch.from_numpy(self.SEQ))


def test_self_critical_batch_and_its_sign():
    """reward = the number of 7s.  The batch is the one train_step takes; a sample above its baseline has a POSITIVE weight on its nll
    — the step minimises sum w nll, so descent raises that sample's likelihood (checked on a toy policy, not by convention)"""
    from mic_amd.evaluation import scst_advantages, self_critical_batch, sequences_to_score_inputs

    model, px = _GenStub(), np.zeros((2, 8, 8, 3), np.float32)
    seen = []

    def reward_fn(seq):
        seen.append(seq)
        return (seq == 7).sum(1)

    b, rewards = self_critical_batch(model, px, reward_fn, 3, prng_key=17, max_length=6, top_k=50)
    assert model.kw == dict(do_sample=True, num_return_sequences=3, prng_key=17, max_length=6, top_k=50, num_beams=1)
    assert len(seen) == 1 and isinstance(seen[0], np.ndarray) and np.array_equal(seen[0], model.SEQ)
    assert rewards.dtype == np.float32 and np.array_equal(rewards, [3, 1, 0, 0, 1, 2])
    assert set(b) == {"pixel_values", "input_ids", "attention_mask", "decoder_input_ids", "captions_per_image", "loss_weights"}
    dec_in, labels, mask = sequences_to_score_inputs(model.SEQ, 2, 1)
    assert b["pixel_values"] is px and b["captions_per_image"] == 3
    assert np.array_equal(b["input_ids"], labels) and np.array_equal(b["attention_mask"], mask) and np.array_equal(b["decoder_input_ids"], dec_in)
    adv = scst_advantages(rewards, 3)
    assert b["loss_weights"].dtype == np.float32 and np.array_equal(b["loss_weights"], adv)  # + advantage, not its negative
    assert b["loss_weights"][0] > 0 > b["loss_weights"][2]                               # the best sample of image 0, and its worst
    from mic_amd.train import check_loss_weights
    assert check_loss_weights(b) is not None
    # the sign, on a toy policy: one logit vector per caption row over {this caption, anything else}; nll = -log softmax[0]
    theta = torch.zeros(6, 2, requires_grad=True)
    nll = -torch.log_softmax(theta, -1)[:, 0]
    (torch.from_numpy(b["loss_weights"]) * nll).sum().backward()
    with torch.no_grad():
        after = torch.log_softmax(theta - 0.5 * theta.grad, -1)[:, 0]
    before = float(np.log(0.5))
    for r in range(6):
        if adv[r] > 0:
            assert after[r] > before, r   # above the baseline: more likely after a descent step
        elif adv[r] < 0:
            assert after[r] < before, r
    # explicit baselines reach scst_advantages; reward_fn's mistakes are refused
    b2, _ = self_critical_batch(model, px, reward_fn, 3, prng_key=0, max_length=6, baseline=np.array([1.0, 1.0]))
    assert np.allclose(b2["loss_weights"], [2, 0, -1, -1, 0, 1])
    with pytest.raises(ValueError, match="rewards"):
        self_critical_batch(model, px, lambda s: np.zeros(5), 3, prng_key=0)
    with pytest.raises(ValueError, match="non-finite"):
        self_critical_batch(model, px, lambda s: np.full(6, np.nan), 3, prng_key=0)


# ------------------------------------------------------------------------------------------------ refusals
R, T = 4, 6
BAD = [
    ("shape", np.ones(R + 1, np.float32)),
    ("shape", np.ones((R, T + 1), np.float32)),
    ("shape", np.ones((T, R), np.float32)),
    ("shape", np.ones((R, T, 1), np.float32)),
    ("shape", np.float32(1.0)),
    ("shape", torch.ones(R * T)),
    ("non-finite", np.array([1.0, np.nan, 1.0, 1.0])),
    ("non-finite", np.array([1.0, 1.0, np.inf, 1.0], np.float32)),
    ("non-finite", torch.full((R, T), float("-inf"))),
    ("real numbers", np.array(["a", "b", "c", "d"])),
    ("real numbers", np.ones(R, np.complex64)),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_refusals_come_before_any_device_work(i):
    from mic_amd.train import check_loss_weights

    word, w = BAD[i]
    b = _batch(2, R, T, captions_per_image=2, loss_weights=w)
    with pytest.raises(ValueError, match=word):
        check_loss_weights(b)
    tr = _trainer()
    for step in (tr.train_step, tr.eval_step):
        with pytest.raises(ValueError, match=word):
            step(b)


def test_accepted_weights_and_the_fp8_refusal():
    from mic_amd.engine import Engine
    from mic_amd.train import check_loss_weights

    assert check_loss_weights(_batch(R, R, T)) is None
    for w in (np.array([1.5, -0.75, 0.0, -0.0]), [1, 2, 3, 4], np.ones((R, T), np.float64), torch.ones(R, dtype=torch.float64)):
        got = check_loss_weights(_batch(R, R, T, loss_weights=w))
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape in ((R,), (R, T))
    b = _batch(R, R, T, loss_weights=np.ones(R, np.float32))
    with pytest.raises(ValueError, match="gemm_dtype='fp8'"):
        check_loss_weights(b, fp8=True)
    assert check_loss_weights(_batch(R, R, T), fp8=True) is None  # without the key fp8 is today's step
    tr = _trainer(fp8=True)
    for step in (tr.train_step, tr.eval_step):
        with pytest.raises(ValueError, match="gemm_dtype='fp8'"):
            step(b)
    with pytest.raises(AssertionError, match="moved to the device"):  # an accepted batch goes on to the device: the stub says so
        _trainer().eval_step(b)
    # the engine's own refusals, before any launch
    eng = Engine.__new__(Engine)
    eng.fp8, eng.dev = True, torch.device("cpu")
    eng._check_row_weights(None, 5)
    with pytest.raises(ValueError, match="fp8"):
        eng._check_row_weights(torch.ones(5), 5)
    eng.fp8 = False
    eng._check_row_weights(torch.ones(5), 5)
    for bad in (torch.ones(4), torch.ones(5, dtype=torch.float64), torch.ones(5, 1), torch.ones(10)[::2], np.ones(5, np.float32)):
        with pytest.raises(ValueError, match="row_weights"):
            eng._check_row_weights(bad, 5)


# ------------------------------------------------------------------------------------------------ header
def test_header_declares_the_weighted_entry_points():
    from mic_amd import _lib as L

    text = open(os.path.join(ROOT, "include", "mic_hip.h")).read()
    for name, nargs in (("mic_ce_reduce_w", 7), ("mic_ce_bwd_w", 14), ("mic_ce_bwd_t_w", 17)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/mic_hip.h"
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == nargs and "const float* row_weight" in args, (name, args)
        assert len(L._SIGS[name][0]) == nargs, name  # the ctypes binding passes as many arguments as the header declares
    assert "mic_ce_bwd_q8_w" not in text  # the fp8 form has no weighted twin


# ------------------------------------------------------------------------------------------------ the GPU tests' fixture
def test_fixture_weights_hide_no_gradient_leaf():
    """tests/test_loss_weights_gpu.py compares the leaves whose reference gradient is not analytically zero (< 1e-6): with this
    fixture that set is the same with and without the weights — 18 of 100 leaves, 82 compared — so the rule cannot hide a leaf
    the weights reach"""
    from oracle import model_ref as M
    from util_small import ref_config

    rc = ref_config("tanh", 1e-6)
    p = M.init_params(rc, seed=1234, perturb_ln=True)
    px, labels, mask, dec_in, w = LW.fixture(rc)
    assert tuple(px.shape[:1]) == (LW.N_IMG,) and tuple(labels.shape) == (LW.N_IMG * LW.G, LW.T) and len({int(x) for x in mask.sum(1)}) > 2
    pxr = px.repeat_interleave(LW.G, 0)
    for ls in (0.0, 0.1):
        zero = []
        for weights in (None, w):
            _, g = LW.loss_and_grads(rc, p, pxr, labels, mask, dec_in, weights, None, ls)
            zero.append({k for k, v in g.items() if v.abs().max().item() < LW.ZERO_LEAF})
            assert len(g) == 100
        assert zero[0] == zero[1], (ls, sorted(zero[0] ^ zero[1]))
        assert len(zero[0]) == 18 and 100 - len(zero[0]) == 82, (ls, len(zero[0]))
