"""Per-caption loss weights through the engine and the Trainer on the GPU (batch["loss_weights"], Engine row_weights), on the fixture
of tests/util_loss_weights_ref.py: 2 images x 3 ragged captions of 12 positions, weights (1.5, -0.75, 0, 2, -1, 0.25).

Every comparison is against the autograd oracle with the weighted loss (util_loss_weights_ref.loss_and_grads), or against the
product's own plain step, under the bounds the existing suites apply to the same quantities of the plain step: tests/
test_captions_per_image_gpu.py (loss 2e-5 and gradient leaves 5e-4 of their scale in fp32; 2e-2 / 8e-2 / cosine 0.995 in bf16),
tests/test_accumulate_gpu.py and tests/test_clip_gpu.py (two optimizer steps: loss 5e-5, grad_norm 5e-4, weights 2e-5)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_loss_weights_ref as LW  # noqa: E402
from test_captions_per_image_gpu import bdict, engine_args, grad_distances, oracle_masks  # noqa: E402
from util_small import batch, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu
N_IMG, G, T = LW.N_IMG, LW.G, LW.T
B = N_IMG * G


def head_weights(model, w, mask, compact):
    """the fp32 device vector over the head's rows: per-caption weights broadcast over T, at the loss rows when the head is compacted"""
    flat = np.repeat(np.asarray(w, np.float32), T) if np.ndim(w) == 1 else np.asarray(w, np.float32).reshape(-1)
    if compact:
        flat = flat[np.nonzero(mask.numpy().reshape(-1))[0]]
    return torch.from_numpy(np.ascontiguousarray(flat)).to(model.device)


def wdict(px, labels, mask, dec_in, w, G=None):
    b = bdict(px, labels, mask, dec_in, G)
    if w is not None:
        b["loss_weights"] = w
    return b


def grouped_batch(rc, seed):
    """the fixture's layout on other seeds: N_IMG images, B ragged captions"""
    px = batch(rc, N_IMG, T, seed=seed)[0]
    _, labels, mask, dec_in = batch(rc, B, T, seed=seed + 1)
    return px, labels, mask, dec_in


# ------------------------------------------------------------------------------------------------------------ fp32, decisive
@pytest.mark.parametrize("train,ls,compact", [(False, 0.0, False), (True, 0.0, False), (True, 0.1, False), (True, 0.1, True), (False, 0.0, True)])
def test_fp32_loss_and_grads_match_the_weighted_oracle(dev, train, ls, compact):
    """Engine.loss_and_grads / loss_only with row_weights, images = n_img: loss 2e-5, every compared leaf 5e-4 of its scale, at least
    82 leaves compared (tests/test_loss_weights_cpu.py: the weights hide none)"""
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    px, labels, mask, dec_in, w = LW.fixture(rc)
    seed = 4242 if train else None
    masks = oracle_masks(model, rc, seed, B, T) if train else None
    pxr = px.repeat_interleave(G, 0)
    ref_loss, ref_g = LW.loss_and_grads(rc, p, pxr, labels, mask, dec_in, w, masks, ls)
    plain = LW.loss_and_grads(rc, p, pxr, labels, mask, dec_in, None, None, ls)[0] if not train else None
    args, kw = engine_args(model, px, labels, mask, dec_in, compact=compact, pack=False, G=G)
    rw = head_weights(model, w, mask, compact)
    loss = model.engine.loss_and_grads(*args, label_smoothing=ls, seed=seed, images=N_IMG, row_weights=rw, **kw)
    torch.cuda.synchronize()
    print(f"[loss_weights fp32 train={train} ls={ls} compact={compact}] loss {loss.item():.7f} oracle {ref_loss.item():.7f}")
    assert abs(loss.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item())), (loss.item(), ref_loss.item())
    if plain is not None:
        assert abs(ref_loss.item() - plain.item()) > 0.1  # (the weighted loss is another number)
    got = model.store.export_flat("grad")
    worst, _ = grad_distances(got, ref_g)
    for k, rg in ref_g.items():
        if rg.abs().max().item() < LW.ZERO_LEAF:
            assert np.abs(got[k]).max() < 1e-6, k
    print(f"  {len(worst)} leaves compared; worst:", sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    assert len(worst) >= 82, len(worst)
    bad = {k: v for k, v in worst.items() if v > 5e-4}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    ref_eval = LW.loss_and_grads(rc, p, pxr, labels, mask, dec_in, w, None, ls)[0] if train else ref_loss
    ev = model.engine.loss_only(*args, label_smoothing=ls, images=N_IMG, row_weights=rw, **kw)
    assert abs(ev.item() - ref_eval.item()) < 2e-5 * max(1.0, abs(ref_eval.item())), (ev.item(), ref_eval.item())


def test_a_weight_of_zero_drops_the_captions_loss_but_not_its_tokens(dev):
    """caption 2 has weight 0: its rows of dlogits are +0 bits, and loss and gradient are those of the reference in which that
    caption's per-token loss is dropped while its tokens stay in the denominator (a per-token weight tensor, zero on caption 2)"""
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    px, labels, mask, dec_in, w = LW.fixture(rc)
    assert w[2] == 0
    w01 = np.ones(B, np.float32)
    w01[2] = 0.0
    keep = torch.ones(B, T)
    keep[2] = 0.0
    ref_loss, ref_g = LW.loss_and_grads(rc, p, px.repeat_interleave(G, 0), labels, mask, dec_in, keep)
    # spelled out: the numerator loses caption 2, the denominator keeps all valid tokens
    from oracle import model_ref, train_ref
    with torch.no_grad():
        logits = model_ref.forward_logits(rc, p, px.repeat_interleave(G, 0), dec_in, mask, None, None)
        m2 = mask.clone()
        m2[2] = 0
        dropped = train_ref.loss_fn(logits, labels, m2) * m2.sum() / mask.sum()
    assert abs(dropped.item() - ref_loss.item()) < 1e-5
    for compact in (True, False):
        args, kw = engine_args(model, px, labels, mask, dec_in, compact=compact, pack=False, G=G)
        loss = model.engine.loss_and_grads(*args, images=N_IMG, row_weights=head_weights(model, w01, mask, compact), **kw)
        torch.cuda.synchronize()
        assert abs(loss.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item())), (loss.item(), ref_loss.item())
        worst, _ = grad_distances(model.store.export_flat("grad"), ref_g)
        bad = {k: v for k, v in worst.items() if v > 5e-4}
        assert len(worst) >= 82 and not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
        dl = model.engine.buf("d.logits", B * T, model.store.Vpad)  # the logits buffer holds dlogits after the backward pass
        pos = np.nonzero(mask.numpy().reshape(-1))[0] if compact else np.arange(B * T)
        mine = torch.from_numpy(pos // T == 2).to(dev)
        live = torch.from_numpy((pos // T != 2) & (mask.numpy().reshape(-1)[pos] != 0)).to(dev)
        rows = dl[:len(pos)]
        assert int(mine.sum()) > 0 and not rows[mine].view(torch.int32).any(), "the rows of the caption of weight 0 are not +0 bits"
        assert (rows[live][:, :rc.vocab_size] != 0).any(1).all()


# ------------------------------------------------------------------------------------------------------------ weights of 1.0
ATOMIC = ("shared", "dec.pos", "flb")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_weights_of_one_are_the_plain_step(dev, dtype):
    """two train steps with loss_weights = ones against a twin Trainer without the key (same weights, seed, batches, dropout 0.1);
    bf16: packed rows and a vocabulary wide enough for the NT head (mic_ce_bwd_t_w), fp32: mic_ce_bwd_w.
    Step 1 starts from identical state: the same loss bits, and the same bytes in every gradient segment and every weight the step
    produces reproducibly.  The segments summed with fp32 atomics in an order that changes between two runs of the SAME call (the
    embedding scatters into `shared` / `dec.pos`, `flb`, the bias / LayerNorm region behind ParamStore.atomic_begin — tests/
    test_captions_per_image_gpu.py::test_default_path_gives_the_same_bits) are compared within 1e-5 of their scale, the size of such
    a reordering.  Step 2 starts from weights that differ by that noise in those segments, so no implementation could give equal bits
    there: it is held to what tests/test_accumulate_gpu.py::test_accumulate_steps_1_is_the_default_trainer holds two runs of the
    same launches to — losses to 1e-5, weights within 2.5 lr per step and all but a sliver within 1e-6."""
    from mic_amd import Trainer, create_learning_rate_fn

    lr = 1e-3
    over = dict(vocab_size=16400) if dtype == torch.bfloat16 else {}
    runs = {}
    for form in ("plain", "ones"):
        rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1, **over)
        tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 0, lr), weight_decay=0.01, seed=3, label_smoothing_factor=0.1)
        st = model.store
        steps = []
        for s in range(2):
            px, labels, mask, dec_in = grouped_batch(rc, 55 + 2 * s)
            w = np.ones(B, np.float32) if form == "ones" else None
            out = tr.train_step(wdict(px, labels, mask, dec_in, w, G))
            torch.cuda.synchronize()
            nt = any(isinstance(k, tuple) and k[0] == "d.dlogitsT" for k in model.engine._bufs)  # the transposing CE backward's output
            assert nt == (dtype == torch.bfloat16) and (tr._pack is not None) == nt  # bf16: packed rows and the NT head
            steps.append((np.float32(float(out["loss"])).tobytes(), float(out["loss"]), st.grad.cpu().numpy().copy(), st.master.cpu().numpy().copy()))
        runs[form] = steps
    exact = 0
    (lb0, _, g0, w0), (lb1, _, g1, w1) = runs["plain"][0], runs["ones"][0]
    assert lb0 == lb1, "step 1: loss bits differ"
    for name, seg in st.segs.items():
        sl = slice(seg.offset, seg.offset + seg.numel)
        if name in ATOMIC or seg.offset >= st.atomic_begin:
            assert np.abs(g1[sl] - g0[sl]).max() <= 1e-5 * max(np.abs(g0[sl]).max(), 1e-12), name
        else:
            exact += 1
            assert g1[sl].tobytes() == g0[sl].tobytes(), f"{name}: gradient bytes differ from the plain step"
            assert w1[sl].tobytes() == w0[sl].tobytes(), f"{name}: weights after step 1 differ from the plain step"
    assert exact >= 20
    l0, l1 = [s[1] for s in runs["plain"]], [s[1] for s in runs["ones"]]
    print(f"[loss_weights ones {dtype}] losses {l1} vs plain {l0}; {exact} segments byte-equal")
    assert np.allclose(l1, l0, rtol=1e-5), (l1, l0)
    diff = np.abs(runs["ones"][1][3] - runs["plain"][1][3])
    assert diff.max() <= 2.5 * lr * 2, diff.max()
    assert (diff > 1e-6).mean() < 1e-3, (diff > 1e-6).mean()


# ------------------------------------------------------------------------------------------------------------ bf16 Trainer
_REF = {}


def fixture_oracle(rc, p):
    """(loss, grads) of the weighted oracle on the fixture at the initial parameters, no dropout: computed once, shared, never modified"""
    if "fixture" not in _REF:
        px, labels, mask, dec_in, w = LW.fixture(rc)
        l, g = LW.loss_and_grads(rc, p, px.repeat_interleave(G, 0), labels, mask, dec_in, w)
        _REF["fixture"] = (l.item(), g)
    return _REF["fixture"]


def _lr():
    from mic_amd import create_learning_rate_fn

    return create_learning_rate_fn(64, 2, 4, 0, 1e-3)


@pytest.mark.parametrize("grouped", [True, False])
@pytest.mark.parametrize("pack", [True, False])
def test_bf16_trainer_step_matches_the_weighted_oracle(dev, pack, grouped):
    """Trainer.train_step in bf16 with the fixture's weights, packed and padded, G = 3 and G = 1 on repeated pixels, against the fp32
    oracle: the bf16 bounds of test_captions_per_image_gpu._check_bf16 — loss 2e-2, every leaf 8e-2 of its scale, cosine > 0.995"""
    from mic_amd import Trainer

    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    px, labels, mask, dec_in, w = LW.fixture(rc)
    ref_loss, ref_g = fixture_oracle(rc, p)
    tr = Trainer(model, _lr(), pack_rows=pack)
    b = wdict(px, labels, mask, dec_in, w, G) if grouped else wdict(px.repeat_interleave(G, 0), labels, mask, dec_in, w)
    loss = float(tr.train_step(b)["loss"])
    torch.cuda.synchronize()
    assert (tr._pack is not None) == pack and (tr._images == N_IMG) == grouped
    worst, cos = grad_distances(model.store.export_flat("grad"), ref_g)
    print(f"[loss_weights bf16 pack={pack} grouped={grouped}] loss {loss:.5f} oracle {ref_loss:.5f}; worst leaf {max(worst.values()):.4f} cos {cos:.5f}")
    assert abs(loss - ref_loss) < 2e-2 * max(1.0, abs(ref_loss)), (loss, ref_loss)
    bad = {k: v for k, v in worst.items() if v > 8e-2}
    assert len(worst) >= 82 and not bad and cos > 0.995, (sorted(bad.items(), key=lambda kv: -kv[1])[:8], cos)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_per_token_weights_equal_to_the_broadcast_give_the_same_bits(dev, dtype):
    """[R, T] weights that repeat each caption's weight over its positions against the [R] form: the same head-row vector, so the same
    loss bits, and the same gradient bytes wherever the step is reproducible (see test_weights_of_one_are_the_plain_step); a host
    array and a device tensor alike"""
    from mic_amd import Trainer

    runs = []
    for form in ("caption", "token", "token_device"):
        rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        tr = Trainer(model, _lr(), seed=3)
        px, labels, mask, dec_in, w = LW.fixture(rc)
        wt = np.repeat(w[:, None], T, 1)
        wt = {"caption": w, "token": wt, "token_device": torch.from_numpy(wt).to(dev)}[form]
        out = tr.train_step(wdict(px, labels, mask, dec_in, wt, G))
        torch.cuda.synchronize()
        runs.append((np.float32(float(out["loss"])).tobytes(), model.store.grad.cpu().numpy()))
    st = model.store
    for lb, g in runs[1:]:
        assert lb == runs[0][0], "loss bits differ"
        for name, seg in st.segs.items():
            sl = slice(seg.offset, seg.offset + seg.numel)
            if name in ATOMIC or seg.offset >= st.atomic_begin:
                assert np.abs(g[sl] - runs[0][1][sl]).max() <= 1e-5 * max(np.abs(runs[0][1][sl]).max(), 1e-12), name
            else:
                assert g[sl].tobytes() == runs[0][1][sl].tobytes(), name
    # and per-token weights that are NOT a broadcast are honoured: the eval loss against the oracle's
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    tr = Trainer(model, _lr())
    px, labels, mask, dec_in, w = LW.fixture(rc)
    wt = (np.repeat(w[:, None], T, 1) * np.linspace(0.5, 1.5, T)[None, :]).astype(np.float32)
    ref = LW.loss_and_grads(rc, p, px.repeat_interleave(G, 0), labels, mask, dec_in, torch.from_numpy(wt))[0].item()
    got = float(tr.eval_step(wdict(px, labels, mask, dec_in, wt, G))["loss"])
    assert abs(got - ref) < 2e-5 * max(1.0, abs(ref)), (got, ref)


# ------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("case", ["accumulate", "clip"])
def test_two_weighted_optimizer_steps_follow_the_oracle(dev, case):
    """fp32, two optimizer steps under a warm-up schedule with accumulate_steps = 2 (four micro-batches) or max_grad_norm = 1.0, every
    batch weighted: the oracle's AdamW steps on the weighted (mean / clipped) gradients.  Bounds of
    test_two_accumulated_steps_match_oracle_adamw and test_two_clipped_steps_match_oracle_adamw_under_warmup: loss 5e-5, grad_norm
    5e-4, every weight 2e-5."""
    from mic_amd import Trainer, create_learning_rate_fn
    from mic_amd.params import flatten_tree
    from oracle import train_ref
    from util_clip import clip_factor, norm64

    N = 2 if case == "accumulate" else 1
    kw = dict(accumulate_steps=2) if case == "accumulate" else dict(max_grad_norm=1.0)
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    lr_fn = create_learning_rate_fn(train_ds_size=40, train_batch_size=4, num_train_epochs=1, num_warmup_steps=2, learning_rate=1e-3)
    tr = Trainer(model, lr_fn, weight_decay=0.01, seed=42, bucket_mb=0.25, **kw)
    params = {k: v.clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(v) for k, v in p.items()}
    w = np.asarray(LW.WEIGHTS, np.float32)
    for step in range(2):
        lr = train_ref.linear_warmup_decay(step, 1e-3, 2, 10)
        losses, grads = [], []
        for j in range(N):
            px, labels, mask, dec_in = grouped_batch(rc, 300 + 2 * (N * step + j))
            wj = np.roll(w, N * step + j)
            l, g = LW.loss_and_grads(rc, params, px.repeat_interleave(G, 0), labels, mask, dec_in, wj)
            out = tr.train_step(wdict(px, labels, mask, dec_in, wj, G))
            losses.append(l.item())
            grads.append(g)
            assert tr.step == step + (1 if j == N - 1 else 0) and abs(float(out["learning_rate"]) - lr) < 1e-9
        mean = sum(losses) / N
        assert abs(float(out["loss"]) - mean) < 5e-5 * max(1.0, abs(mean)), (float(out["loss"]), mean)
        gm = {k: sum(g[k] for g in grads) / N for k in params}
        f = 1.0
        if case == "clip":
            n_ref = norm64(gm)
            assert abs(float(out["grad_norm"]) - n_ref) <= 5e-4 * n_ref, (float(out["grad_norm"]), n_ref)
            f = clip_factor(n_ref, 1.0)
            assert f < 0.8  # (the clip is active)
        for k in params:
            params[k], m[k], v[k] = train_ref.adamw_update(params[k], f * gm[k], m[k], v[k], step, lr, wd=0.01)
    gf = flatten_tree(model.params)
    worst = max(((torch.from_numpy(gf[k]).reshape(rv.shape) - rv).abs().max().item(), k) for k, rv in params.items())
    print(f"[loss_weights {case}] largest parameter difference {worst}")
    assert worst[0] < 2e-5, worst


def test_eval_step_honours_the_weights(dev):
    """loss only, fp32 (2e-5) and bf16 packed (2e-2), against the weighted oracle; without the key it is the plain loss"""
    from mic_amd import Trainer

    for dtype, tol in ((torch.float32, 2e-5), (torch.bfloat16, 2e-2)):
        rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
        px, labels, mask, dec_in, w = LW.fixture(rc)
        ref = fixture_oracle(rc, p)[0]
        tr = Trainer(model, _lr())
        got = float(tr.eval_step(wdict(px, labels, mask, dec_in, w, G))["loss"])
        plain = float(tr.eval_step(wdict(px, labels, mask, dec_in, None, G))["loss"])
        print(f"[loss_weights eval {dtype}] {got:.6f} oracle {ref:.6f} (plain {plain:.6f})")
        assert abs(got - ref) < tol * max(1.0, abs(ref)), (got, ref)
        assert abs(plain - ref) > 0.1


# ------------------------------------------------------------------------------------------------------------ the loop, end to end
def test_self_critical_batch_end_to_end(dev):
    """sample 3 captions per image, reward them on the host, take the step: the returned batch passes train_step and the step's loss
    is the definition evaluated by the oracle on that batch (fp32, no dropout: 2e-5)"""
    from mic_amd import Trainer
    from mic_amd.evaluation import self_critical_batch
    from oracle import model_ref

    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    px = batch(rc, N_IMG, T, seed=11)[0]
    reward_fn = lambda seq: (seq >= 500).sum(1)  # noqa: E731  deterministic: the number of ids in the upper half of the vocabulary
    b, rewards = self_critical_batch(model, px.numpy(), reward_fn, 3, prng_key=5, max_length=12)
    R = N_IMG * 3
    assert rewards.shape == (R,) and b["captions_per_image"] == 3 and b["input_ids"].shape == (R, 11) and b["loss_weights"].shape == (R,)
    assert np.abs(b["loss_weights"]).max() > 0, rewards  # (the samples of an image did not all earn the same)
    labels, mask, dec_in = (torch.from_numpy(np.asarray(b[k]).astype(np.int64)) for k in ("input_ids", "attention_mask", "decoder_input_ids"))
    with torch.no_grad():
        logits = model_ref.forward_logits(rc, p, px.repeat_interleave(3, 0), dec_in, mask, None, None)
        ref = LW.weighted_loss_fn(logits, labels, mask, b["loss_weights"]).item()
    tr = Trainer(model, _lr())
    out = tr.train_step(b)
    torch.cuda.synchronize()
    print(f"[self_critical_batch] rewards {rewards.tolist()} weights {b['loss_weights'].tolist()} loss {float(out['loss']):.7f} reference {ref:.7f}")
    assert tr.step == 1 and tr._images == N_IMG
    assert abs(float(out["loss"]) - ref) < 2e-5 * max(1.0, abs(ref)), (float(out["loss"]), ref)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_device_work(dev, monkeypatch):
    from mic_amd import Trainer

    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    px, labels, mask, dec_in, w = LW.fixture(rc)
    tr = Trainer(model, _lr())

    def no_device(*a, **k):
        raise AssertionError("the batch was moved to the device before the refusal")

    monkeypatch.setattr(model, "_dev", no_device)
    nan = w.copy()
    nan[1] = np.nan
    for word, bad in (("shape", w[:-1]), ("shape", np.ones((B, T + 1), np.float32)), ("shape", torch.ones(B + 1, device=dev)), ("non-finite", nan)):
        for step in (tr.train_step, tr.eval_step):
            with pytest.raises(ValueError, match=word):
                step(wdict(px, labels, mask, dec_in, bad, G))
    monkeypatch.undo()
    # the engine: a vector of another length than the head's rows, before any launch
    args, kw = engine_args(model, px, labels, mask, dec_in, compact=True, pack=False, G=G)
    for fn in (model.engine.loss_and_grads, model.engine.loss_only):
        with pytest.raises(ValueError, match="row_weights"):
            fn(*args, images=N_IMG, row_weights=torch.ones(B * T, device=dev), **kw)
    assert tr.step == 0
    # fp8 GEMMs: the Trainer and the engine refuse the weights; the plain step still runs
    rc, p, model8 = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    tr8 = Trainer(model8, _lr(), gemm_dtype="fp8")
    pxr = px.repeat_interleave(G, 0)
    monkeypatch.setattr(model8, "_dev", no_device)
    for step in (tr8.train_step, tr8.eval_step):
        with pytest.raises(ValueError, match="gemm_dtype='fp8'"):
            step(wdict(pxr, labels, mask, dec_in, w))
    monkeypatch.undo()
    args, kw = engine_args(model8, pxr, labels, mask, dec_in, compact=True, pack=False, G=1)
    n = kw["rows"][1]
    for fn in (model8.engine.loss_and_grads, model8.engine.loss_only):
        with pytest.raises(ValueError, match="fp8"):
            fn(*args, row_weights=torch.ones(n, device=dev), **kw)
    assert np.isfinite(float(tr8.train_step(wdict(pxr, labels, mask, dec_in, None))["loss"]))
