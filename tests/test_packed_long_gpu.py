"""Packed decoder rows beyond one 64x64 attention tile: seq_len > 64 and more than 64 encoder positions, through
Engine.loss_and_grads / loss_only and Trainer.train_step / eval_step, against the padded rows on the same batch.  The reduced model
(bf16 storage, dropout 0) and the bounds of test_packed_decoder_rows_edge_lengths and
test_trainer_packs_rows_by_default_and_matches_the_padded_trainer (tests/test_model_gpu.py), and of
test_fp8_fused_emission_equals_the_quantiser_path_also_beyond_one_attention_tile (tests/test_fp8_gpu.py).

The loss is compared bit for bit, as at one tile: a valid query row walks the same key blocks on packed and on padded rows (causal:
blocks 0 .. its own; cross-attention: all of them), every key it admits is the same stored value, and a padded key inside its last
block is excluded by the causal rule on both sides — so every valid row of the final hidden state has the same bits, and the
compacted head sees the same rows."""
import numpy as np
import pytest
import torch

from util_small import batch, make_pair

pytestmark = pytest.mark.gpu

LONG = dict(gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0, max_position_embeddings=256)


def _batch_of(rc, lens, T, seed):
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    px = torch.randn(B, rc.image_size, rc.image_size, 3, generator=g).clamp(-1.8, 2.2)
    labels = torch.full((B, T), rc.pad_token_id, dtype=torch.int64)
    mask = torch.zeros((B, T), dtype=torch.int64)
    for b, n in enumerate(lens):
        labels[b, :n] = torch.randint(4, rc.vocab_size - 20, (n,), generator=g)
        mask[b, :n] = 1
    dec_in = torch.full_like(labels, rc.pad_token_id)
    dec_in[:, 1:] = labels[:, :-1]
    return px, labels, mask, dec_in


def _both(model, px, labels, mask, dec_in, T):
    """(loss, gradients) of Engine.loss_and_grads and the loss of Engine.loss_only on packed rows and on padded rows, same batch, same
    compacted head"""
    from mic_amd import loss_rows, packed_rows

    d, dev, B = model._dev, model.device, labels.shape[0]
    pos = torch.arange(T, dtype=torch.int32, device=dev)[None].expand(B, T).contiguous()
    idx, rl = loss_rows(mask.numpy(), labels.numpy())
    kw = dict(rows=(d(idx, torch.int32), len(idx)), row_labels=d(rl, torch.int32))
    q_off, q_len, ids_p, pos_p = (d(t, torch.int32) for t in packed_rows(mask.numpy(), dec_in.numpy()))
    lp = float(model.engine.loss_and_grads(d(px, torch.float32), ids_p, pos_p, None, d(labels, torch.int32).reshape(-1), B, T,
                                           pack=(q_off, q_len, len(idx)), **kw))
    gp = {k: v.copy() for k, v in model.store.export_flat("grad").items()}
    ep = float(model.engine.loss_only(d(px, torch.float32), ids_p, pos_p, None, d(labels, torch.int32).reshape(-1), B, T,
                                      pack=(q_off, q_len, len(idx)), **kw))
    er = float(model.engine.loss_only(d(px, torch.float32), d(dec_in, torch.int32).reshape(-1), pos.reshape(-1), d(mask, torch.int32),
                                      d(labels, torch.int32).reshape(-1), B, T, **kw))
    lr = float(model.engine.loss_and_grads(d(px, torch.float32), d(dec_in, torch.int32).reshape(-1), pos.reshape(-1), d(mask, torch.int32),
                                           d(labels, torch.int32).reshape(-1), B, T, **kw))
    gr = model.store.export_flat("grad")
    return lp, gp, (ep, er), lr, gr


def _compare(lp, gp, ev, lr, gr, what):
    assert np.isfinite(lp) and lp == lr, (what, lp, lr)
    assert np.isfinite(ev[0]) and ev[0] == ev[1], (what, "loss_only", ev)
    for k in gr:
        sc = max(np.abs(gr[k]).max(), 1e-12)
        assert np.abs(gp[k] - gr[k]).max() <= 2e-4 * sc, (what, k, np.abs(gp[k] - gr[k]).max() / sc)


def _three_batches(lens):
    """the lengths as given, then two batches with fewer valid rows on the same buffers: what the longer batch left behind the valid
    rows must not count"""
    return [list(lens), [max(1, n // 2) for n in reversed(lens)], [max(1, n - 37) for n in lens]]


@pytest.mark.parametrize("T,lens", [(72, [1, 72, 64, 65, 2, 71]), (130, [130, 1, 129, 64, 65])])
def test_engine_packed_rows_beyond_one_tile_match_the_padded_rows(dev, T, lens):
    rc, p, model = make_pair(torch.bfloat16, dev, **LONG)
    counts = set()
    for seed, ls in enumerate(_three_batches(lens)):
        counts.add(sum(ls))
        _compare(*_both(model, *_batch_of(rc, ls, T, seed=T + seed), T), what=(T, ls))
    assert len(counts) == 3


def test_engine_packed_rows_with_more_than_64_encoder_positions(dev):
    """T = 16 over 8x8 patches + the class token = 65 encoder positions: the cross-attention K / V span two key blocks (tiled packed
    cores), the self-attention stays on the one-tile packed cores"""
    rc, p, model = make_pair(torch.bfloat16, dev, image_size=128, **LONG)
    assert rc.v_seq == 65 and model.store.S == 65
    counts = set()
    for seed, ls in enumerate(_three_batches([1, 16, 2, 15, 16, 1, 3])):
        counts.add(sum(ls))
        _compare(*_both(model, *_batch_of(rc, ls, 16, seed=160 + seed), 16), what=(16, ls))
    assert len(counts) == 3


def test_trainer_packs_rows_beyond_one_tile_and_matches_the_padded_trainer(dev):
    """three train steps and one eval step at T = 72, pack_rows=True against False.  Losses and eval loss: the bounds of the seq-12
    Trainer test (first loss bit for bit, then rtol 2e-3).  Parameters: Adam's normalised update turns a gradient difference at a
    ~0 gradient into at most lr per element and step (tests/test_model_gpu.py, the optimizer-stream test: 2.5 lr per step)."""
    from mic_amd import Trainer, create_learning_rate_fn

    T, lr, steps, res = 72, 1e-3, 3, {}
    for pack in (True, False):
        rc, p, model = make_pair(torch.bfloat16, dev, **LONG)
        tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 0, lr), pack_rows=pack)
        losses = []
        for s in range(steps):
            px, labels, mask, dec_in = batch(rc, 4, T, seed=70 + s)
            b = {"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}
            losses.append(float(tr.train_step(b)["loss"]))
            assert (tr._pack is not None) == pack
        ev = float(tr.eval_step(b)["loss"])
        assert (tr._pack is not None) == pack
        torch.cuda.synchronize()
        res[pack] = (losses, ev, model.store.master.clone())
    assert np.isfinite(res[True][0]).all() and res[True][0][0] == res[False][0][0]  # first step: same weights, same loss bit for bit
    assert np.allclose(res[True][0], res[False][0], rtol=2e-3) and abs(res[True][1] - res[False][1]) < 2e-3 * abs(res[False][1])
    diff = (res[True][2] - res[False][2]).abs().max().item()
    assert diff <= 2.5 * lr * steps, diff


def _packed_pass(model, px, labels, mask, dec_in, T):
    from mic_amd import loss_rows, packed_rows

    d, B = model._dev, labels.shape[0]
    idx, rl = loss_rows(mask.numpy(), labels.numpy())
    q_off, q_len, ids_p, pos_p = (d(t, torch.int32) for t in packed_rows(mask.numpy(), dec_in.numpy()))
    loss = model.engine.loss_and_grads(d(px, torch.float32), ids_p, pos_p, None, d(labels, torch.int32).reshape(-1), B, T,
                                       pack=(q_off, q_len, len(idx)), rows=(d(idx, torch.int32), len(idx)), row_labels=d(rl, torch.int32))
    torch.cuda.synchronize()
    return loss.item(), {k: v.copy() for k, v in model.store.export_flat("grad").items()}


def test_fp8_fused_emission_equals_the_quantiser_path_on_packed_rows_beyond_one_tile(dev):
    """three passes on one batch at T = 72 on packed rows, the producers emitting the fp8 operands (from pass 2 on) against every
    operand through the quantiser (`f8.fused = False`): the tiled attention backward has no fp8 form on packed rows either, its
    dQ / dK / dV go through the quantiser.  Bounds of the padded-row test: loss 1e-5, gradients 2e-4."""
    T, res = 72, {}
    for fused in (True, False):
        rc, p, model = make_pair(torch.bfloat16, dev, **LONG)
        model.engine.set_gemm_dtype("fp8")
        model.engine.f8.fused = fused
        px, labels, mask, dec_in = batch(rc, 3, T, seed=21)
        res[fused] = [_packed_pass(model, px, labels, mask, dec_in, T) for _ in range(3)]
        if fused:
            assert len(model.engine._a8_ready) > 20
    for (la, ga), (lb, gb) in zip(res[True], res[False]):
        assert np.isfinite(la) and abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
        for k in ga:
            a, b = ga[k].astype(np.float64), gb[k].astype(np.float64)
            assert np.abs(a - b).max() <= 2e-4 * max(np.abs(a).max(), 1e-30), (k, np.abs(a - b).max(), np.abs(a).max())
