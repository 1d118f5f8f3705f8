"""References of the per-row loss weights (batch["loss_weights"], Engine row_weights, mic_ce_*_w), built on what exists.  A helper
module, not a conftest.

The one definition (include/mic_hip.h, Trainer.train_step): loss = sum_{r,t} w[r,t] m[r,t] l[r,t] / sum_{r,t} m[r,t] — the
denominator is the mask count whatever the weights are.

Kernel level: tests/util_rowop_ref.py's fp64 references with the row factor mask * weight in place of mask.  The bounds are its
bounds with |w| replaced by |w weight| plus ONE more fp32 rounding (U32) of that factor for the extra multiply:
    reduce   (gamma_R + 2 u32 + u32) sum|l mask weight| / denom + EPS_F |loss|
    dlogits  ce_bwd_ref is linear in its loss_scale argument and its bound is |w| (..) + (EPS_F + u32) |v|, so row r of the weighted
             reference is ce_bwd_ref's row at loss_scale 1 times s_r = loss_scale weight[r]: v = s_r v1,
             e = |s_r| e1 + u32 |v| before storage (e1: the fp32 bound, storage applied afterwards for the dtype).
Model level: oracle.train_ref.loss_fn restated with a weight tensor, fed by oracle.model_ref.forward_logits under autograd."""
from __future__ import annotations

import math

import numpy as np
import torch

import util_rowop_ref as RR
from util_gemm_ref import EPS_F, U32, gamma_k

# the fixture of the model-level tests: n_img images, G captions each, T positions; one weight per caption — a value above 1,
# negatives, a zero, distinct magnitudes
N_IMG, G, T = 2, 3, 12
WEIGHTS = (1.5, -0.75, 0.0, 2.0, -1.0, 0.25)
ZERO_LEAF = 1e-6  # a gradient leaf whose reference magnitude is below this is analytically zero (tests/test_captions_per_image_gpu.py)


# ------------------------------------------------------------------------------------------------ kernel level
def ce_reduce_w_ref(row_loss, mask, weight):
    """(loss, bound, denom) of mic_ce_reduce_w"""
    l, m, w = (np.asarray(a, np.float64) for a in (row_loss, mask, weight))
    den = m.sum()
    f = m * w
    loss = (l * f).sum() / den
    return loss, (gamma_k(len(l)) + 3 * U32) * np.abs(l * f).sum() / den + EPS_F * abs(loss) + 1e-300, den


def ce_bwd_w_ref(x, V, labels, mask, weight, ls, lse, denom, loss_scale, dtype):
    """(dlogits [rows][Vpad], bound) of mic_ce_bwd_w / mic_ce_bwd_t_w on stored logits x [rows][Vpad]"""
    v1, e1 = RR.ce_bwd_ref(x, V, labels, mask, ls, lse, denom, 1.0, "f32")  # (f32 storage: u32 |v| + (1 + u32) e — undone below)
    e1 = (e1 - U32 * np.abs(v1)) / (1 + U32)
    s = (float(np.float32(loss_scale)) * np.asarray(weight, np.float64))[:, None]
    v = s * v1
    e = np.abs(s) * e1 + U32 * np.abs(v)
    return v, RR.stored(None, dtype)(v, e)


def kernel_weights(rows, mask, seed=0):
    """distinct per-row fp32 weights with +0, -0, negatives, a value above 1 and a nonzero weight on a mask-0 row; returns
    (weights float32, rows whose factor is zero)"""
    rng = np.random.default_rng(1000 + seed)
    w = (rng.permutation(rows) + 1).astype(np.float64) / rows * 1.75 + 0.125  # distinct, in (0.125, 1.875]
    w[rng.random(rows) < 0.4] *= -1.0
    w = w.astype(np.float32)
    on = np.nonzero(np.asarray(mask) != 0)[0]
    off = np.nonzero(np.asarray(mask) == 0)[0]
    assert len(on) >= 4 and len(off) >= 1
    w[on[0]], w[on[1]], w[on[2]], w[on[3]] = np.float32(0.0), np.float32(-0.0), np.float32(-2.25), np.float32(2.5)
    w[off[0]] = np.float32(3.0)
    assert np.signbit(w[on[1]]) and not np.signbit(w[on[0]]) and len(set(w.view(np.uint32).tolist())) == rows
    return w, (np.asarray(mask) == 0) | (w == 0)


# ------------------------------------------------------------------------------------------------ model level
def weighted_loss_fn(logits, labels, padding_mask, weights, label_smoothing_factor=0.0):
    """oracle.train_ref.loss_fn (main.py:658-680) with a weight per position: weights [B] (per caption) or [B, T]; the same
    statements in the same order, `m * w` in place of `m` in the numerator — all weights 1.0 give loss_fn's bits"""
    vocab = logits.shape[-1]
    confidence = 1.0 - label_smoothing_factor
    low = (1.0 - confidence) / (vocab - 1)
    if confidence < 1.0:
        norm_const = -(confidence * math.log(confidence) + (vocab - 1) * low * math.log(low + 1e-20))
    else:
        norm_const = 0.0
    logp = torch.log_softmax(logits.to(torch.float32), dim=-1)
    nll_label = -logp.gather(-1, labels.to(torch.int64)[..., None])[..., 0]
    loss = confidence * nll_label + low * (-logp.sum(-1) - nll_label) if low > 0 else nll_label
    loss = loss - norm_const
    m = padding_mask.to(torch.float32)
    w = torch.as_tensor(weights, dtype=torch.float32)
    w = w[:, None].expand_as(m) if w.dim() == 1 else w
    return (loss * (m * w)).sum() / m.sum()


def loss_and_grads(cfg, params, pixel_values, labels, attention_mask, decoder_input_ids, weights, masks=None, label_smoothing_factor=0.0):
    """oracle.train_ref.loss_and_grads with the weighted loss (weights None: train_ref's own)"""
    from oracle import model_ref, train_ref

    if weights is None:
        return train_ref.loss_and_grads(cfg, params, pixel_values, labels, attention_mask, decoder_input_ids, masks, label_smoothing_factor)
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    logits = model_ref.forward_logits(cfg, leaves, pixel_values, decoder_input_ids, attention_mask, None, masks)
    loss = weighted_loss_fn(logits, labels, attention_mask, weights, label_smoothing_factor)
    loss.backward()
    return loss.detach(), {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}


def fixture(rc):
    """(pixels [N_IMG], labels, mask, dec_in [N_IMG * G, T], weights float32 [N_IMG * G]) of the model-level tests"""
    from util_small import batch

    px = batch(rc, N_IMG, T, seed=11)[0]
    _, labels, mask, dec_in = batch(rc, N_IMG * G, T, seed=12)
    return px, labels, mask, dec_in, np.asarray(WEIGHTS, np.float32)
