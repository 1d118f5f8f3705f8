"""generate(num_return_sequences=N) on the GPU, reduced model (tests/util_small.py).

Sampling (float32): N draws per image from one decode chain = N separate `generate(prng_key=keys[n])` calls = the oracle's `sample`
on keys[n], token ids bit for bit, in the reference's raw-logits mode and in the processed mode; `scores` = the log-likelihood of each
caption as drawn, against fp64 from the oracle's recorded logits within 2 (L - 1) 2e-4 max|logit| (the project's fp32 logit bound, once
for the drawn logit and once for the normaliser, per step).  bfloat16: shape, id range, PAD after the end, forced tokens, finite
scores only (grouped and separate calls run their GEMMs at different row counts there; the kernel's bf16 arithmetic is covered in
tests/test_sample_keyed_gpu.py).

Beam search (float32): the N best of the K final hypotheses against `util_nreturn_ref.beam_search_all` on the oracle, scores within
1e-4, row 0 of every image bitwise the plain call; with languages and a shortlist bitwise the separate calls."""
import numpy as np
import pytest
import torch

from util_nreturn_ref import RecordingStepper, beam_search_all, draw_keys, n_best, sample_scored
from util_small import batch, make_pair

pytestmark = pytest.mark.gpu

B, L = 3, 9
BOS = 996
WARP = dict(top_k=20, top_p=0.9, temperature=0.7)


@pytest.fixture(scope="module")
def fp32(dev):
    """(oracle config, oracle params, product model, images, oracle encoder states)"""
    from oracle import model_ref as M

    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    px = batch(rc, B, 8, seed=4)[0]
    with torch.no_grad():
        ehs, _ = M.encode(rc, p, px)
    yield rc, p, model, px, ehs
    model.release_decode_plans()


def _set_eos_bias(rc, p, model, bias):
    from mic_amd.params import unflatten_tree

    p = dict(p)
    flb = p["final_logits_bias"].clone()
    flb[0, rc.eos_token_id] = bias
    p["final_logits_bias"] = flb
    if model is not None:
        model.params = unflatten_tree({k: v.numpy() for k, v in p.items()})
    return p


def _oracle_draws(rc, p, ehs, prng_key, N, mode, *, min_length=0, forced_bos=BOS, max_length=L):
    """per draw n: the oracle's `sample` on keys[n] (ids), and sample_scored on the same key: (ids, fp64 scores, steps, max |logit|)"""
    from oracle import generation_ref as G

    procs = G.get_logits_processor(min_length, max_length, rc.eos_token_id, forced_bos, rc.eos_token_id)
    warpers = G.get_logits_warper(WARP["top_k"], WARP["top_p"], WARP["temperature"]) if mode else []
    out = []
    for key in draw_keys(prng_key, N):
        args = (B, 2, max_length, rc.pad_token_id, rc.eos_token_id, key, procs, warpers)
        ref = G.sample(G.ModelStepper(rc, p, ehs, max_length), *args, sample_from_processed_logits=mode)
        rec = RecordingStepper(G.ModelStepper(rc, p, ehs, max_length))
        seq, scores, steps = sample_scored(rec, *args, mode)
        assert np.array_equal(seq, ref)  # the scored loop is the oracle's loop
        out.append((ref, scores, steps, max(float(np.abs(x).max()) for x in rec.logits)))
    return out


def _check_sampled(rc, model, px, out, refs, N, max_length=L):
    seq, scores = out.sequences.cpu().numpy(), out.scores.cpu().numpy()
    assert seq.shape == (B * N, max_length) and seq.dtype == np.int32 and scores.shape == (B * N,) and scores.dtype == np.float32
    worst = 0.0
    for n, (ref, ref_scores, steps, scale) in enumerate(refs):
        assert np.array_equal(seq[n::N], ref), (n, seq[n::N], ref)  # row image * N + n
        tol = 2 * (max_length - 1) * 2e-4 * scale
        d = float(np.abs(scores[n::N].astype(np.float64) - ref_scores).max())
        print(f"[nreturn] draw {n}/{N}: max |score - fp64| {d:.3g} (tolerance {tol:.3g}, scores {ref_scores.min():.3f} .. {ref_scores.max():.3f}, {steps} steps)")
        assert d <= tol, (n, d, tol)
        worst = max(worst, d / tol)
    return worst


@pytest.mark.parametrize("mode", [False, True])
@pytest.mark.parametrize("N", [2, 3, 4])
def test_draws_equal_separate_calls_and_the_oracle(fp32, N, mode):
    rc, p, model, px, ehs = fp32
    kw = dict(max_length=L, do_sample=True, num_beams=1, forced_bos_token_id=BOS, sample_from_processed_logits=mode, **WARP)
    out = model.generate(px, prng_key=123, num_return_sequences=N, **kw)
    refs = _oracle_draws(rc, p, ehs, 123, N, mode)
    _check_sampled(rc, model, px, out, refs, N)
    seq = out.sequences.cpu().numpy()
    for n, key in enumerate(draw_keys(123, N)):
        one = model.generate(px, prng_key=key, **kw)
        assert "scores" not in one  # the plain call is what it was
        assert np.array_equal(one.sequences.cpu().numpy(), seq[n::N]), n
    if mode:
        assert (seq[:, 1] == BOS).all()
    assert len({seq[i].tobytes() for i in range(N)}) > 1  # the draws of an image differ
    # prng_key None is PRNGKey(0), and a 2-word key passes through
    a = model.generate(px, num_return_sequences=N, **kw)
    b = model.generate(px, prng_key=np.array([0, 0], dtype=np.uint32), num_return_sequences=N, **kw)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.scores, b.scores)
    assert np.array_equal(a.sequences.cpu().numpy()[0::N], _oracle_draws(rc, p, ehs, 0, N, mode)[0][0])


def test_draws_that_finish_at_different_steps(dev, fp32):
    """EOS pushed up through final_logits_bias on model and oracle; the bias is chosen on the CPU with the oracle such that the draws'
    own calls stop at different steps and all of them before max_length: the rows of a call that has stopped ride along"""
    rc, p0, _, px, ehs = fp32
    N, chosen = 3, None
    for bias in (5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0, 9.0):
        p = _set_eos_bias(rc, p0, None, bias)
        refs = _oracle_draws(rc, p, ehs, 7, N, False)
        steps = [r[2] for r in refs]
        if len(set(steps)) > 1 and max(steps) < L - 1:
            chosen = bias
            break
    assert chosen is not None, "no EOS bias makes the draws stop at different steps before max_length"
    print(f"[nreturn] EOS bias {chosen}: the draws' calls stop after {steps} steps")
    _, _, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    _set_eos_bias(rc, p0, model, chosen)
    out = model.generate(px, max_length=L, do_sample=True, num_beams=1, prng_key=7, num_return_sequences=N, forced_bos_token_id=BOS)
    _check_sampled(rc, model, px, out, refs, N)
    seq = out.sequences.cpu().numpy()
    assert (seq[:, max(steps) + 1:] == rc.pad_token_id).all()
    model.release_decode_plans()


def test_min_length_and_forced_tokens(fp32):
    rc, p, model, px, ehs = fp32
    N = 2
    out = model.generate(px, max_length=L, do_sample=True, num_beams=1, prng_key=77, num_return_sequences=N, min_length=4, forced_bos_token_id=BOS,
                         forced_eos_token_id=rc.eos_token_id, sample_from_processed_logits=True, **WARP)
    refs = _oracle_draws(rc, p, ehs, 77, N, True, min_length=4)
    _check_sampled(rc, model, px, out, refs, N)
    seq = out.sequences.cpu().numpy()
    assert (seq[:, 1] == BOS).all() and all(r[2] >= 5 for r in refs)  # forced BOS; no call ends while cur_len <= min_length
    assert (seq[:, L - 1] == rc.pad_token_id).all()  # forced EOS at the last step -> finished -> PAD


def test_warm_plan_with_graphs_follows_the_key(fp32, monkeypatch):
    """MIC_DECODE_GRAPHS=1: call 1 of the plan runs eagerly, call 2 captures the steps and replays them, call 3 only replays — each
    with another prng_key, each its own key's oracle result: the keys are read from the plan's device table"""
    rc, p, model, px, ehs = fp32
    monkeypatch.setenv("MIC_DECODE_GRAPHS", "1")
    model.release_decode_plans()
    N = 2
    kw = dict(max_length=L, do_sample=True, num_beams=1, num_return_sequences=N, forced_bos_token_id=BOS, sample_from_processed_logits=True, **WARP)
    seen = []
    for call, key in enumerate((11, 12, 13)):
        out = model.generate(px, prng_key=key, **kw)
        plan = next(iter(model._decode_plans.values()))
        assert len(model._decode_plans) == 1 and plan.calls == call + 1
        if call >= 1:
            assert len(plan.graphs) > 0
        _check_sampled(rc, model, px, out, _oracle_draws(rc, p, ehs, key, N, True), N)
        seen.append(out.sequences.cpu().numpy().tobytes())
    assert len(set(seen)) == 3
    monkeypatch.setenv("MIC_DECODE_GRAPHS", "0")
    eager = model.generate(px, prng_key=13, **kw)
    assert torch.equal(eager.sequences, out.sequences) and torch.equal(eager.scores, out.scores)
    model.release_decode_plans()


def test_bf16_sampled_captions_are_well_formed(dev):
    """final_logits_bias pushes EOS up (rows finish early and at different steps) and takes PAD out of reach (-1e9: no draw can be PAD,
    so a PAD in a row can only be the bookkeeping's): from its first PAD on a row holds nothing but PAD"""
    from mic_amd.params import unflatten_tree

    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6)
    p = dict(p)
    flb = p["final_logits_bias"].clone()
    flb[0, rc.eos_token_id], flb[0, rc.pad_token_id] = 6.0, -1e9
    p["final_logits_bias"] = flb
    model.params = unflatten_tree({k: v.numpy() for k, v in p.items()})
    px = batch(rc, B, 8, seed=4)[0]
    N = 4
    for mode in (False, True):
        out = model.generate(px, max_length=L, do_sample=True, num_beams=1, prng_key=5, num_return_sequences=N, forced_bos_token_id=BOS,
                             sample_from_processed_logits=mode, **WARP)
        seq, scores = out.sequences.cpu().numpy(), out.scores.cpu().numpy()
        assert seq.shape == (B * N, L) and scores.shape == (B * N,)
        assert (seq >= 0).all() and (seq < rc.vocab_size).all() and (seq[:, 0] == 2).all()
        assert np.isfinite(scores).all() and (scores <= 0).all()
        is_pad = seq[:, 1:] == rc.pad_token_id
        first = np.where(is_pad.any(1), is_pad.argmax(1), L - 1)  # index (in seq[:, 1:]) of a row's first PAD, L - 1 for none
        for r, row in enumerate(seq):
            assert rc.eos_token_id not in row[1:].tolist()  # the EOS draw itself is written as PAD
            assert (row[1 + first[r]:] == rc.pad_token_id).all(), (mode, r, row)  # PAD after the end, and nothing else
        print(f"[nreturn] bf16 {'processed' if mode else 'raw'}: rows end after {sorted(first.tolist())} tokens")
        assert (first < L - 2).sum() >= 3  # rows did finish early: the check is not vacuous
        if mode:
            assert (seq[:, 1] == BOS).all() and (seq[:, L - 1] == rc.pad_token_id).all()  # forced BOS; forced EOS -> PAD
        else:
            assert len(set(first.tolist())) > 1  # ... and at different steps
    model.release_decode_plans()


# ------------------------------------------------------------------------------------------------ beam search: the N best of K
K = 4


def _oracle_beams(rc, p, ehs, max_length=L, **kw):
    from oracle import generation_ref as G

    procs = G.get_logits_processor(kw.get("min_length", 0), max_length, rc.eos_token_id, kw.get("forced_bos", BOS), kw.get("forced_eos", rc.eos_token_id))
    return beam_search_all(G.ModelStepper(rc, p, ehs.repeat_interleave(K, 0), max_length), B, K, 2, max_length, rc.pad_token_id, rc.eos_token_id,
                           1.0, True, procs)


@pytest.mark.parametrize("N", [1, 2, 4])
def test_n_best_hypotheses_against_the_oracle(fp32, N):
    rc, p, model, px, ehs = fp32
    kw = dict(max_length=L, num_beams=K, forced_bos_token_id=BOS)
    plain = model.generate(px.numpy(), **kw)
    out = model.generate(px.numpy(), num_return_sequences=N, **kw)
    all_seq, all_scores, steps = _oracle_beams(rc, p, ehs)
    ref_seq, ref_scores = n_best(all_seq, all_scores, N)
    seq, scores = out.sequences.cpu().numpy(), out.scores.cpu().numpy()
    assert seq.shape == (B * N, L) and scores.shape == (B * N,) and out["steps"] == steps == plain["steps"]
    assert np.array_equal(seq, ref_seq), (seq, ref_seq)
    # the existing beam-score bound, in the form tests/test_generate_gpu.py::test_beam_ids_exact states it (finished scores carry the
    # reference's -1e7 arithmetic, hence the relative term)
    assert np.allclose(scores, ref_scores, rtol=1e-4, atol=1e-4), np.abs(scores - ref_scores).max()
    assert torch.equal(out.sequences[0::N], plain.sequences) and torch.equal(out.scores[0::N], plain.scores)  # row j = 0: bitwise the plain call
    assert (np.diff(scores.reshape(B, N), axis=1) <= 0).all()  # best first


def test_nothing_finished_returns_the_running_hypotheses(fp32):
    """L = 4 with min_length = 4 and no forced EOS: EOS is suppressed at every step, no hypothesis finishes"""
    rc, p, model, px, ehs = fp32
    mc = model.config.mbart_config
    keep = mc.forced_eos_token_id
    mc.forced_eos_token_id = None
    try:
        out = model.generate(px.numpy(), max_length=4, min_length=4, num_beams=K, num_return_sequences=K, forced_bos_token_id=BOS)
        plain = model.generate(px.numpy(), max_length=4, min_length=4, num_beams=K, forced_bos_token_id=BOS)
    finally:
        mc.forced_eos_token_id = keep
    all_seq, all_scores, steps = _oracle_beams(rc, p, ehs, 4, min_length=4, forced_eos=None)
    ref_seq, ref_scores = n_best(all_seq, all_scores, K)
    seq, scores = out.sequences.cpu().numpy(), out.scores.cpu().numpy()
    # running hypotheses: no EOS after the start token (which has the same id), no -1e7 arithmetic
    assert not (ref_seq[:, 1:] == rc.eos_token_id).any() and (ref_scores > -1e5).all()
    assert np.array_equal(seq, ref_seq) and np.allclose(scores, ref_scores, rtol=1e-4, atol=1e-4) and out["steps"] == steps
    assert torch.equal(out.sequences[0::K], plain.sequences) and torch.equal(out.scores[0::K], plain.scores)


def test_languages_and_shortlist_equal_the_separate_calls(fp32):
    rc, p, model, px, ehs = fp32
    N, ids = 2, [996, 995]
    rng = np.random.default_rng(0)
    A = np.unique(np.concatenate([rng.choice(rc.vocab_size, 300, replace=False), [rc.eos_token_id] + ids]))
    for extra in (dict(), dict(allowed_token_ids=A)):
        kw = dict(max_length=L, num_beams=K, num_return_sequences=N, **extra)
        out = model.generate(px.numpy(), forced_bos_token_id=ids, **kw)
        assert tuple(out.sequences.shape) == (2, B * N, L) and tuple(out.scores.shape) == (2, B * N) and len(out["steps"]) == 2
        for g, bos in enumerate(ids):
            one = model.generate(px.numpy(), forced_bos_token_id=bos, **kw)
            assert tuple(one.sequences.shape) == (B * N, L)
            assert torch.equal(one.sequences, out.sequences[g]) and torch.equal(one.scores, out.scores[g]) and one["steps"] == out["steps"][g]
        if extra:
            assert np.isin(out.sequences.cpu().numpy()[:, :, 1:], np.concatenate([A, [rc.pad_token_id]])).all()
    from mic_amd.evaluation import generate_languages

    got = generate_languages(model, px.numpy(), {"a": 996, "b": 995}, max_length=L, num_beams=K, num_return_sequences=N)
    assert got["a"].shape == (B * N, L)
    plainer = model.generate(px.numpy(), forced_bos_token_id=ids, max_length=L, num_beams=K, num_return_sequences=N)
    assert np.array_equal(got["a"], plainer.sequences.cpu().numpy()[0]) and np.array_equal(got["b"], plainer.sequences.cpu().numpy()[1])


def test_sliced_search_returns_the_same_n_best(fp32, monkeypatch):
    rc, p, model, px, ehs = fp32
    px4 = torch.cat([px, px[:1] * 0.5])
    kw = dict(max_length=L, num_beams=K, num_return_sequences=3, forced_bos_token_id=BOS)
    monkeypatch.setenv("MIC_DECODE_SLICES", "1")
    one = model.generate(px4.numpy(), **kw)
    monkeypatch.setenv("MIC_DECODE_SLICES", "2")
    cut = model.generate(px4.numpy(), **kw)
    assert tuple(cut.sequences.shape) == (4 * 3, L)
    assert torch.equal(one.sequences, cut.sequences) and torch.equal(one.scores, cut.scores) and one["steps"] == cut["steps"]
    model.release_decode_plans()
