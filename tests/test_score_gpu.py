"""model.score on the GPU: teacher-forced caption log-likelihoods against the oracle's logits (fp32), against the evaluation pass whose
row losses it shares (bf16), several candidates per image against the repeated-image pass, against the `scores` generate sums along
its decode chain, arbitrary 0/1 masks, and that the logits-free head allocates no logits.

The model is the small pair widened to d_model 256 (K = 256: the head reaches gemm_d2_kernel<2>); the batch is 3 images x 3
candidates, T = 16, ragged, row 0 of full length."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from util_small import batch, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu

N_IMG, G, T = 3, 3, 16
R = N_IMG * G
WIDE = dict(d_model=256, d_ffn=512, d_heads=4)


def _pair(dtype, dev):
    return make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0, **WIDE)


def _batch(rc):
    px = batch(rc, N_IMG, T, seed=40)[0]
    _, labels, mask, dec_in = batch(rc, R, T, seed=41)
    assert mask[0].all() and len({int(n) for n in mask.sum(1)}) > 3  # one full-length row, ragged
    return px, labels, mask, dec_in


@pytest.fixture(scope="module")
def fp32(dev):
    rc, p, model = _pair(torch.float32, dev)
    yield rc, p, model
    model.release_decode_plans()


@pytest.fixture(scope="module")
def bf16(dev):
    return _pair(torch.bfloat16, dev)


@pytest.fixture(scope="module")
def oracle_logprobs(fp32):
    """fp64 log-softmax of the oracle's logits at the labels [R, T] (computed once, read-only)"""
    from oracle import model_ref as M

    rc, p, _ = fp32
    px, labels, mask, dec_in = _batch(rc)
    with torch.no_grad():
        logits = M.forward_logits(rc, p, px.repeat_interleave(G, 0), dec_in, mask)
    lp = torch.log_softmax(logits.double(), -1).gather(2, labels[..., None])[..., 0]
    lp.requires_grad_(False)
    return lp.numpy()


def _np(t):
    return t.detach().cpu().numpy()


def _head_is_free(model, rows):
    return model.engine.score_head_free(rows)


# ------------------------------------------------------------------------------------------------ fp32 against the oracle
def test_fp32_matches_the_oracle(fp32, oracle_logprobs):
    rc, p, model = fp32
    px, labels, mask, dec_in = _batch(rc)
    out = model.score(px.numpy(), labels.numpy(), mask.numpy(), decoder_input_ids=dec_in.numpy(), candidates_per_image=G, return_token_logprobs=True)
    m = mask.numpy().astype(bool)
    ref_tok = np.where(m, oracle_logprobs, 0.0)
    tok, ll, nt = _np(out.token_logprobs), _np(out.log_likelihood), _np(out.num_tokens)
    assert tok.shape == (R, T) and tok.dtype == np.float32 and ll.shape == (R,) and ll.dtype == np.float32 and nt.dtype == np.int32
    print(f"[score fp32] max |token logprob - oracle| {np.abs(tok - ref_tok).max():.3g}; max |ll - oracle| {np.abs(ll - ref_tok.sum(1)).max():.3g}")
    assert np.array_equal(nt, m.sum(1))
    assert (tok[~m] == 0).all()
    assert np.allclose(tok, ref_tok, rtol=1e-4, atol=1e-4)
    n = m.sum(1)
    assert (np.abs(ll - ref_tok.sum(1)) <= 1e-4 * n + 1e-4 * np.abs(ref_tok).sum(1)).all()
    # the defaults: mask from the pad id, decoder inputs from shift_tokens_right — this batch is built that way
    dflt = model.score(px.numpy(), labels.numpy(), candidates_per_image=G)
    assert "token_logprobs" not in dflt and torch.equal(dflt.log_likelihood, out.log_likelihood) and torch.equal(dflt.num_tokens, out.num_tokens)


# ------------------------------------------------------------------------------------------------ bf16 against the evaluation pass
@pytest.mark.parametrize("g", [1, 3])
def test_bf16_shares_its_row_losses_with_eval_step(bf16, g, monkeypatch):
    from mic_amd import Trainer, create_learning_rate_fn

    rc, p, model = bf16
    px, labels, mask, dec_in = _batch(rc)
    pxg = px if g == G else px.repeat_interleave(G, 0)
    b = {"pixel_values": pxg.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}
    if g > 1:
        b["captions_per_image"] = g
    tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 0, 1e-3), seed=7)
    loss = float(tr.eval_step(b)["loss"])
    assert tr._pack is not None  # default packing
    monkeypatch.delenv("MIC_SCORE_HEAD", raising=False)
    assert _head_is_free(model, int(mask.sum()))
    out = model.score(pxg.numpy(), labels.numpy(), mask.numpy(), decoder_input_ids=dec_in.numpy(), candidates_per_image=g, return_token_logprobs=True)
    ll, nt = _np(out.log_likelihood).astype(np.float64), _np(out.num_tokens)
    N = int(nt.sum())
    mine = -ll.sum() / N
    print(f"[score bf16 G={g}] eval_step loss {loss:.8f}, -sum(ll)/N {mine:.8f}, relative {abs(mine - loss) / abs(loss):.3g} (bound {2 * N * 2.0 ** -24:.3g})")
    assert N == int(mask.sum()) and abs(mine - loss) <= 2 * N * 2.0 ** -24 * abs(loss)
    # the materialised head (A/B switch, read at call time): the same token bits
    monkeypatch.setenv("MIC_SCORE_HEAD", "materialised")
    assert not _head_is_free(model, N)
    mat = model.score(pxg.numpy(), labels.numpy(), mask.numpy(), decoder_input_ids=dec_in.numpy(), candidates_per_image=g, return_token_logprobs=True)
    assert torch.equal(mat.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32))
    assert torch.equal(mat.log_likelihood.view(torch.int32), out.log_likelihood.view(torch.int32))


# ------------------------------------------------------------------------------------------------ several candidates per image
@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_candidates_per_image_against_repeated_images(request, which):
    """the bounds of tests/test_captions_per_image_gpu.py for the shared path against the repeated-image path: 2e-5 (fp32) and 2e-2
    (bf16) of max(1, |value|)"""
    rc, p, model = request.getfixturevalue(which)
    px, labels, mask, dec_in = _batch(rc)
    kw = dict(decoder_input_ids=dec_in.numpy(), return_token_logprobs=True)
    shared = model.score(px.numpy(), labels.numpy(), mask.numpy(), candidates_per_image=G, **kw)
    rep = model.score(px.repeat_interleave(G, 0).numpy(), labels.numpy(), mask.numpy(), candidates_per_image=1, **kw)
    tol = 2e-5 if which == "fp32" else 2e-2
    for key in ("log_likelihood", "token_logprobs"):
        a, b = _np(shared[key]).astype(np.float64), _np(rep[key]).astype(np.float64)
        print(f"[score G={G} vs repeated, {which}] {key}: max distance {np.abs(a - b).max():.3g}")
        assert (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))).all(), key
    assert torch.equal(shared.num_tokens, rep.num_tokens)
    with pytest.raises(ValueError, match="images need"):
        model.score(px.repeat_interleave(G, 0).numpy(), labels.numpy(), mask.numpy(), candidates_per_image=G)
    with pytest.raises(ValueError, match="images need"):
        model.score(px[:2].numpy(), labels.numpy(), mask.numpy(), candidates_per_image=G)


# ------------------------------------------------------------------------------------------------ against generate (fp32)
def test_scores_of_generate_are_the_scores_of_score(dev):
    """sampling from the raw logits with no processor in force sums log p(token) along the KV-cached decode chain; score() computes
    the same quantity in one teacher-forced pass.  The EOS bias and the key are chosen on the CPU oracle such that rows stop at EOS
    before max_length and rows run into it."""
    from mic_amd.evaluation import rerank, sequences_to_score_inputs
    from mic_amd.params import unflatten_tree
    from oracle import model_ref as M
    from util_nreturn_ref import draw_keys, sample_scored
    from oracle import generation_ref as Gen

    L, N = 12, 3
    rc, p, model = _pair(torch.float32, dev)
    mc = model.config.mbart_config
    px = batch(rc, N_IMG, T, seed=40)[0]
    with torch.no_grad():
        ehs, _ = M.encode(rc, p, px)
    chosen = None
    for bias in (3.0, 2.5, 3.5, 4.0):  # (the start token is EOS: the tied head already favours it at the first step)
        pb = dict(p)
        flb = p["final_logits_bias"].clone()
        flb[0, rc.eos_token_id] = bias
        pb["final_logits_bias"] = flb
        for key in (3, 4, 5, 6):
            refs = [sample_scored(Gen.ModelStepper(rc, pb, ehs, L), N_IMG, mc.decoder_start_token_id, L, rc.pad_token_id, rc.eos_token_id, k, [], [], False)
                    for k in draw_keys(key, N)]
            lens = sequences_to_score_inputs(np.concatenate([seq for seq, _, _ in refs]), rc.eos_token_id, rc.pad_token_id)[2].sum(1)
            never_ended = np.concatenate([(seq != rc.pad_token_id).all(1) for seq, _, _ in refs])
            if ((lens > 1) & (lens < L - 1)).any() and never_ended.any():  # a row that stops midway, a row that never stops
                chosen = (bias, key, pb, refs)
                break
        if chosen:
            break
    assert chosen is not None, "no (EOS bias, key) gives rows that stop at EOS before max_length beside rows that do not"
    bias, key, pb, refs = chosen
    model.params = unflatten_tree({k: v.numpy() for k, v in pb.items()})
    keep = (mc.forced_bos_token_id, mc.forced_eos_token_id, mc.min_length)
    mc.forced_bos_token_id = mc.forced_eos_token_id = mc.min_length = None
    try:
        gen = model.generate(px.numpy(), do_sample=True, num_beams=1, prng_key=key, num_return_sequences=N, max_length=L)
        seq = gen.sequences.cpu().numpy()
        for n, (rseq, _, _) in enumerate(refs):
            assert np.array_equal(seq[n::N], rseq)  # the chain under test is the oracle's chain
        dec_in, labels, mask = sequences_to_score_inputs(seq, rc.eos_token_id, rc.pad_token_id)
        assert (mask.sum(1) < L - 1).any() and (mask.sum(1) == L - 1).any()
        out = model.score(px.numpy(), labels, mask, decoder_input_ids=dec_in, candidates_per_image=N)
        ll, nt, gs = _np(out.log_likelihood).astype(np.float64), _np(out.num_tokens), _np(gen.scores).astype(np.float64)
        print(f"[score vs generate] EOS bias {bias}, key {key}: tokens {nt.tolist()}, max |ll - generate's score| {np.abs(ll - gs).max():.3g}")
        assert np.array_equal(nt, mask.sum(1))
        assert (np.abs(ll - gs) <= 1e-4 * nt + 1e-4 * np.abs(gs)).all(), (ll, gs)
        best, scores = rerank(model, px.numpy(), seq, N, length_penalty=1.0)
        want = (ll / nt).reshape(N_IMG, N)
        assert np.array_equal(best, want.argmax(1)) and np.allclose(scores, want, rtol=1e-6, atol=1e-6)
    finally:
        mc.forced_bos_token_id, mc.forced_eos_token_id, mc.min_length = keep
        model.release_decode_plans()


# ------------------------------------------------------------------------------------------------ arbitrary 0/1 masks
@pytest.mark.parametrize("which", ["fp32", "bf16"])
def test_mask_with_a_hole_takes_the_unpacked_path(request, which):
    """a hole in a row's mask: that position carries no score and is no key for the later ones.  The positions BEFORE the hole see what
    they see under the prefix mask: the same values there (the unpacked pass against the packed one in bf16: the bf16 bound of the
    padded against the packed trainer, 2e-2 of max(1, |value|); fp32: both unpacked, 2e-5), zero at the hole and behind the mask.
    A row without any valid token scores 0 with 0 tokens."""
    rc, p, model = request.getfixturevalue(which)
    px, labels, mask, dec_in = _batch(rc)
    kw = dict(decoder_input_ids=dec_in.numpy(), candidates_per_image=G, return_token_logprobs=True)
    full = model.score(px.numpy(), labels.numpy(), mask.numpy(), **kw)
    holed = mask.clone()
    hole = {0: 9, 2: 1}  # row -> position, inside the rows' valid prefixes (every row has at least 4 valid positions)
    for r, t in hole.items():
        assert mask[r, t + 1] == 1
        holed[r, t] = 0
    holed[4] = 0  # a row with no valid token
    out = model.score(px.numpy(), labels.numpy(), holed.numpy(), **kw)
    tok, ref = _np(out.token_logprobs).astype(np.float64), _np(full.token_logprobs).astype(np.float64)
    tol = 2e-5 if which == "fp32" else 2e-2
    same = holed.numpy().astype(bool).copy()
    for r, t in hole.items():
        same[r, t:] = False  # (positions behind a hole attend one key fewer: another quantity)
    print(f"[score hole {which}] max distance on the shared positions {np.abs(tok - ref)[same].max():.3g}")
    assert (np.abs(tok - ref)[same] <= tol * np.maximum(1.0, np.abs(ref[same]))).all()
    assert (tok[~holed.numpy().astype(bool)] == 0).all() and np.isfinite(tok).all()
    nt, ll = _np(out.num_tokens), _np(out.log_likelihood)
    assert np.array_equal(nt, holed.sum(1).numpy()) and nt[4] == 0 and ll[4] == 0
    assert np.allclose(ll, tok.sum(1), rtol=1e-5, atol=1e-5)
    # all rows empty: nothing to run
    none = model.score(px.numpy(), labels.numpy(), np.zeros_like(mask.numpy()), candidates_per_image=G)
    assert (none.log_likelihood == 0).all() and (none.num_tokens == 0).all()


# ------------------------------------------------------------------------------------------------ no logits buffer
def test_logits_free_score_allocates_no_logits(dev, monkeypatch):
    monkeypatch.delenv("MIC_SCORE_HEAD", raising=False)
    rc, p, model = _pair(torch.bfloat16, dev)
    eng = model.engine
    Vpad = eng.P.Vpad

    def logits_like():
        named = [k for k in eng._bufs if isinstance(k, tuple) and str(k[0]).startswith("d.logits")]
        shaped = [k for k, t in eng._bufs.items() if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[1] >= Vpad and t.dtype == torch.bfloat16
                  and not str(k[0]).startswith("w.") and "ckv" not in str(k[0])]  # (weights; the cross k/v of all layers: L * 2 * d columns)
        return named, shaped

    px, labels, mask, dec_in = _batch(rc)
    model.score(px.numpy(), labels.numpy(), mask.numpy(), candidates_per_image=G)
    assert logits_like() == ([], []), logits_like()
    for rows in (40, 400):  # 40 and then 400 caption rows of one image each
        pxr = batch(rc, rows, T, seed=50)[0]
        _, lab, msk, _ = batch(rc, rows, T, seed=51)
        out = model.score(pxr.numpy(), lab.numpy(), msk.numpy())
        assert torch.isfinite(out.log_likelihood).all() and (out.log_likelihood < 0).all()
        assert logits_like() == ([], []), (rows, logits_like())
    # ... and the materialised form is the one that allocates them
    monkeypatch.setenv("MIC_SCORE_HEAD", "materialised")
    model.score(px.numpy(), labels.numpy(), mask.numpy(), candidates_per_image=G)
    assert logits_like()[0]
