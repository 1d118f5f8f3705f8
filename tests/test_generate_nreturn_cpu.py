"""generate(num_return_sequences=N): the host-only half.  The references of tests/util_nreturn_ref.py against the oracle they extend
(beam search with all K hypotheses, the per-draw key schedule, the counters of a grouped row), `prng.split(key, N)` /
`prng.step_key_table`, and the argument validation — including that what `generate` refuses today keeps its message and that every
refusal comes before the encoder runs.  No GPU."""
import types

import numpy as np
import pytest

from util_nreturn_ref import beam_search_all, counters_of_grouped_row, counters_of_rows, draw_keys, key_schedule, n_best, sample_scored

V, L = 13, 6
START, PAD, EOS = 4, 1, 2


def _table(peak_fn):
    def t(step, hist):
        x = np.linspace(-4.0, -3.0, V).astype(np.float32)  # distinct values: no accidental ties
        for tok, val in peak_fn(step, hist).items():
            x[tok] = val
        return x
    return t


CASES = {
    # every hypothesis of every image may finish; early_stopping off: the loop runs until nothing can improve
    "finishing": dict(peaks=lambda s, h: {2: 1.0 + 0.3 * len(h), 5: 2.0, 6: 1.7, 7: 1.2}, early_stopping=False, length_penalty=1.0, procs=None),
    # early_stopping: the loop ends once an image's K finished slots are full
    "early_stopping": dict(peaks=lambda s, h: {2: 2.5, 5: 2.0, 6: 1.9}, early_stopping=True, length_penalty=0.8, procs=None),
    # EOS can never enter the top-2K: no image has a finished hypothesis, the running ones come back
    "none_finished": dict(peaks=lambda s, h: {5: 2.0, 6: 1.8, 10: 1.0, 2: -1e9}, early_stopping=True, length_penalty=1.0, procs=(0, None, None)),
    # forced BOS and EOS, MinLength
    "processors": dict(peaks=lambda s, h: {2: 2.2, 5: 2.0, 6: 1.9, 8: 1.0}, early_stopping=False, length_penalty=1.2, procs=(3, 11, 2)),
}


def _beam_pair(name, B=2, K=3, rows_differ=False):
    from oracle import generation_ref as G

    c = CASES[name]
    procs = G.get_logits_processor(*((c["procs"][0], L, EOS) + tuple(c["procs"][1:]))) if c["procs"] else []
    tab = _table(c["peaks"])
    if rows_differ:  # image 1 (rows K .. 2K-1) can never emit EOS, image 0 can
        class Stepper(G.ScriptedStepper):
            def step(self, tokens):
                out = super().step(tokens)
                out[K:, EOS] = -1e9
                return out
        mk = lambda: Stepper(B * K, tab)  # noqa: E731
    else:
        mk = lambda: G.ScriptedStepper(B * K, tab)  # noqa: E731
    args = (B, K, START, L, PAD, EOS, c["length_penalty"], c["early_stopping"], procs)
    return G.beam_search(mk(), *args), beam_search_all(mk(), *args)


@pytest.mark.parametrize("name", list(CASES))
def test_beam_search_all_ends_with_the_oracles_best(name):
    ref, (seq, scores, steps) = _beam_pair(name)
    assert seq.shape == (2, 3, L) and scores.shape == (2, 3)
    assert np.array_equal(seq[:, -1], ref.sequences) and np.array_equal(scores[:, -1], ref.scores) and steps == ref.steps
    assert (np.diff(scores, axis=1) >= 0).all()  # sorted ascending, best last
    s2, sc2 = n_best(seq, scores, 2)
    assert np.array_equal(s2[0::2], ref.sequences) and np.array_equal(sc2[0::2], ref.scores)  # row image * N + 0 is the plain result
    assert np.array_equal(s2[1::2], seq[:, -2]) and (sc2[0::2] >= sc2[1::2]).all()


def test_beam_search_all_case_properties():
    """the cases are what their names say"""
    from oracle import generation_ref as G

    _, (seq, scores, steps) = _beam_pair("none_finished")
    assert not (seq == EOS).any() and (scores > -1e5).any() and steps == L - 1
    ref, (seq, scores, steps) = _beam_pair("early_stopping")
    assert steps < L - 1 and (seq == EOS).any(axis=2).all()  # ended early with every slot finished
    # one image finishes, the other never does: its rows are the running hypotheses, the first image's may hold untouched slots
    ref, (seq, scores, steps) = _beam_pair("finishing", rows_differ=True)
    assert np.array_equal(seq[:, -1], ref.sequences) and np.array_equal(scores[:, -1], ref.scores) and steps == ref.steps
    assert (seq[0] == EOS).any() and not (seq[1] == EOS).any()
    # a slot that never held a finished hypothesis: a PAD row with the NEG sentinel, as it lies in the state
    # exactly one hypothesis can ever finish: at cur_len 2, after token 12.  (At cur_len 1 its score (lp - 1e7) / 1 would round to NEG
    # itself and lose the tie against the untouched slots: gen:890, 910 and the index-stable top-k.)
    tab = _table(lambda s, h: {2: 9.0} if len(h) == 2 and h[1] == 12 else {5: 2.0, 2: -1e9})
    seq, scores, _ = beam_search_all(G.ScriptedStepper(3, tab), 1, 3, START, L, PAD, EOS, 1.0, False, [])
    assert (seq[0, -1] == EOS).any() and (seq[0, 0] == PAD).all() and scores[0, 0] == G.NEG


def test_split_and_key_table_follow_the_oracle():
    from mic_amd import prng
    from oracle import generation_ref as G

    for seed in (0, 123, 2 ** 40 + 7):
        for N in (1, 2, 3, 4, 7):
            keys = prng.split(prng.prng_key(seed), N)
            assert keys.dtype == np.uint32 and np.array_equal(keys, G.prng_split(G.prng_key(seed), N))
            assert np.array_equal(keys, draw_keys(seed, N))
    keys = draw_keys(77, 3)
    assert np.array_equal(draw_keys(np.array([0, 77], dtype=np.uint32), 3), keys)
    table = prng.step_key_table(keys, 9)
    assert table.shape == (9, 3, 2) and table.dtype == np.uint32 and np.array_equal(table, key_schedule(keys, 9))
    for n in range(3):  # entry [cur_len][n] is what `sample` draws with at cur_len when started from keys[n]
        key = keys[n]
        for cur_len in range(1, 9):
            k, key = G.prng_split(key)
            assert np.array_equal(table[cur_len, n], k)
    assert len({tuple(k) for k in table[1:].reshape(-1, 2).tolist()}) == 8 * 3  # all different


@pytest.mark.parametrize("images,Vc", [(3, 1003), (4, 1000), (3, 1000), (1, 7), (2, 5)])  # odd and even images * V
@pytest.mark.parametrize("draws", [1, 2, 3])
def test_grouped_rows_use_the_counters_of_their_image(images, Vc, draws):
    """row (image, n) of the grouped launch has the threefry counters of row `image` of a separate call over `images` rows — and
    with them its bits: checked against the oracle's random_bits"""
    from oracle import generation_ref as G

    c0, c1, word = counters_of_rows(images, Vc)
    key = G.prng_key(5 + images)
    bits = G.random_bits(key, images * Vc).reshape(images, Vc)
    for row in range(images * draws):
        g0, g1, gw = counters_of_grouped_row(images, draws, Vc, row)
        image = row // draws
        assert np.array_equal(g0, c0[image]) and np.array_equal(g1, c1[image]) and np.array_equal(gw, word[image])
        a, b = G.threefry2x32(key, g0.astype(np.uint32), g1.astype(np.uint32))
        assert np.array_equal(np.where(gw == 0, a, b), bits[image])


def test_sample_scored_is_the_oracles_sample():
    from oracle import generation_ref as G

    tab = _table(lambda s, h: {3: 1.0, 5: 0.5, 2: 0.8})
    procs = G.get_logits_processor(2, L, EOS, 7, EOS)
    for mode, warpers in ((False, []), (True, G.get_logits_warper(4, 0.9, 0.7))):
        ref = G.sample(G.ScriptedStepper(3, tab), 3, START, L, PAD, EOS, G.prng_key(5), procs, warpers, sample_from_processed_logits=mode)
        seq, scores, steps = sample_scored(G.ScriptedStepper(3, tab), 3, START, L, PAD, EOS, G.prng_key(5), procs, warpers, mode)
        assert np.array_equal(seq, ref) and np.isfinite(scores).all() and (scores <= 0).all() and 1 <= steps <= L - 1
    # a chain of forced tokens only: every step is a point mass
    seq, scores, _ = sample_scored(G.ScriptedStepper(2, tab), 2, START, 3, PAD, EOS, G.prng_key(1), G.get_logits_processor(0, 3, EOS, 7, EOS), [], True)
    assert (seq[:, 1] == 7).all() and (scores == 0).all()


# ------------------------------------------------------------------------------------------------ validation
def _norm(n, **kw):
    from mic_amd.generation_clip_vision_utils import normalize_num_return_sequences

    return normalize_num_return_sequences(n, **kw)


def test_accepted_values():
    assert _norm(None, do_sample=False, num_beams=1) == 1
    assert _norm(None, do_sample=True, num_beams=4) == 1  # without the argument nothing is looked at here
    assert _norm(1, do_sample=False, num_beams=1) == 1
    assert _norm(4, do_sample=False, num_beams=4) == 4 and _norm(np.int64(2), do_sample=False, num_beams=4) == 2
    assert _norm(7, do_sample=True, num_beams=1) == 7  # draws are not bounded by num_beams
    assert _norm(1, do_sample=True, num_beams=1) == 1


@pytest.mark.parametrize("bad", [0, -1, 2.0, 1.5, "2", True, [2], np.array([1, 2])])
def test_not_a_positive_integer(bad):
    for kw in (dict(do_sample=False, num_beams=4), dict(do_sample=True, num_beams=1)):
        with pytest.raises(ValueError, match="num_return_sequences"):
            _norm(bad, **kw)


def test_greedy_and_too_few_beams():
    with pytest.raises(ValueError, match="greedy"):
        _norm(2, do_sample=False, num_beams=1)
    with pytest.raises(ValueError, match="num_beams=4"):
        _norm(5, do_sample=False, num_beams=4)


def test_existing_refusals_keep_their_messages_and_come_first():
    from mic_amd.generation_clip_vision_utils import normalize_allowed_token_ids

    for n in (1, 2, 0, "x"):  # also where the argument itself is malformed
        with pytest.raises(NotImplementedError, match="Beam sampling is currently not implemented"):
            _norm(n, do_sample=True, num_beams=2)
        with pytest.raises(NotImplementedError, match="num_beams > 32"):
            _norm(n, do_sample=False, num_beams=33)
    with pytest.raises(NotImplementedError, match="do_sample=True with `allowed_token_ids` is not implemented"):
        normalize_allowed_token_ids([2, 3, 4], 1003, do_sample=True)


def _stub_model():
    """what generate() touches before the encoder: the generation defaults.  encode() fails the test if it is reached."""
    from mic_amd.generation_clip_vision_utils import FlaxCLIPVisionMBartGenerationMixin

    class Stub(FlaxCLIPVisionMBartGenerationMixin):
        def __init__(self):
            mc = types.SimpleNamespace(max_length=8, bos_token_id=0, pad_token_id=1, eos_token_id=2, decoder_start_token_id=2, do_sample=False,
                                       num_beams=4, max_position_embeddings=64, vocab_size=1003, forced_bos_token_id=None,
                                       forced_eos_token_id=2, min_length=0, length_penalty=1.0, early_stopping=True)
            self.config = types.SimpleNamespace(mbart_config=mc, is_encoder_decoder=True)

        def encode(self, *a, **k):
            raise AssertionError("the encoder ran")
    return Stub()


@pytest.mark.parametrize("kw,err,match", [
    (dict(num_return_sequences=0), ValueError, "num_return_sequences"),
    (dict(num_return_sequences=2.0), ValueError, "num_return_sequences"),
    (dict(num_return_sequences=2, num_beams=1), ValueError, "greedy"),
    (dict(num_return_sequences=5, num_beams=4), ValueError, "exceeds num_beams=4"),
    (dict(num_return_sequences=5), ValueError, "exceeds num_beams=4"),  # num_beams from the config
    (dict(num_return_sequences=2, do_sample=True, num_beams=1, forced_bos_token_id=[996, 995]), NotImplementedError, "sequence of language ids"),
    (dict(num_return_sequences=2, do_sample=True, num_beams=1, allowed_token_ids=[2, 5, 6]), NotImplementedError, "allowed_token_ids"),
    (dict(num_return_sequences=2, do_sample=True, num_beams=2), NotImplementedError, "Beam sampling"),
    (dict(num_return_sequences=2, num_beams=33), NotImplementedError, "num_beams > 32"),
])
def test_generate_refuses_before_the_encoder_runs(kw, err, match):
    with pytest.raises(err, match=match):
        _stub_model().generate(np.zeros((1, 4, 4, 3), np.float32), **kw)


def test_generate_reaches_the_encoder_with_valid_arguments():
    for kw in (dict(num_return_sequences=2), dict(num_return_sequences=4, num_beams=4), dict(num_return_sequences=3, do_sample=True, num_beams=1),
               dict(num_return_sequences=1, num_beams=1)):
        with pytest.raises(AssertionError, match="the encoder ran"):
            _stub_model().generate(np.zeros((1, 4, 4, 3), np.float32), **kw)
