"""Evaluation harness of the reference: the eval loop of `main.py:791-854` / `evaluation.py:142-196` —
per-language `eval_step` loss, beam generation with `decoder_start_token_id = <language code>` (main.py:820) and
BLEU-1..4 over word-tokenised text (`compute_metrics`, main.py:577-603).

The reference scores with `datasets.load_metric("bleu")` (the tensorflow/nmt `compute_bleu`: clipped n-gram counts pooled
over the corpus, geometric mean of the 1..max_order precisions, brevity penalty exp(1 - ref_len/hyp_len) with the SHORTEST
reference length per segment, no smoothing) [UNVERIFIED-3P: restated from the published algorithm; `datasets` cannot fetch
the metric script here] and tokenises with `nltk.word_tokenize` (absent from this image): the tokeniser is a parameter,
default = a Unicode word/punctuation splitter.  All of this is host code; the GPU work is `Trainer.eval_step` and
`model.generate`."""
from __future__ import annotations

import collections
import math
import re
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np

_WORD = re.compile(r"\w+|[^\w\s]", re.UNICODE)


def simple_word_tokenize(text: str, language: Optional[str] = None) -> List[str]:
    """Stand-in for `nltk.word_tokenize(text, language=...)` (main.py:581-584): words and single punctuation marks."""
    return _WORD.findall(text)


def _ngrams(tokens: Sequence[str], max_order: int) -> collections.Counter:
    c = collections.Counter()
    for n in range(1, max_order + 1):
        for i in range(len(tokens) - n + 1):
            c[tuple(tokens[i: i + n])] += 1
    return c


def compute_bleu(predictions: Sequence[Sequence[str]], references: Sequence[Sequence[Sequence[str]]], max_order: int = 4,
                 smooth: bool = False) -> Dict[str, object]:
    """`metric.compute(predictions=..., references=..., max_order=i)` (main.py:596-598): corpus BLEU.
    predictions[i] = token list; references[i] = list of reference token lists."""
    matches, possible = [0] * max_order, [0] * max_order
    ref_len = hyp_len = 0
    for hyp, refs in zip(predictions, references):
        ref_len += min(len(r) for r in refs)
        hyp_len += len(hyp)
        merged = collections.Counter()
        for r in refs:
            merged |= _ngrams(r, max_order)
        overlap = _ngrams(hyp, max_order) & merged
        for ng, cnt in overlap.items():
            matches[len(ng) - 1] += cnt
        for n in range(1, max_order + 1):
            if len(hyp) - n + 1 > 0:
                possible[n - 1] += len(hyp) - n + 1
    precisions = []
    for n in range(max_order):
        if smooth:
            precisions.append((matches[n] + 1.0) / (possible[n] + 1.0))
        else:
            precisions.append(matches[n] / possible[n] if possible[n] > 0 else 0.0)
    geo = math.exp(sum(math.log(p) for p in precisions) / max_order) if min(precisions) > 0 else 0.0
    ratio = hyp_len / ref_len if ref_len > 0 else 0.0
    bp = 1.0 if ratio > 1.0 else (math.exp(1.0 - 1.0 / ratio) if ratio > 0 else 0.0)
    return {"bleu": geo * bp, "precisions": precisions, "brevity_penalty": bp, "length_ratio": ratio,
            "translation_length": hyp_len, "reference_length": ref_len}


def compute_metrics(pred_ids, label_ids, batch_decode: Callable[[Iterable[Sequence[int]]], List[str]],
                    word_tokenize: Callable[[str], List[str]] = simple_word_tokenize) -> Dict[str, float]:
    """main.py:586-603: decode ids (special tokens skipped by `batch_decode`), strip, tokenise, BLEU-1..4."""
    preds = [word_tokenize(p.strip()) for p in batch_decode(pred_ids)]
    labels = [[word_tokenize(l.strip())] for l in batch_decode(label_ids)]
    return {f"BLEU-{i}": compute_bleu(preds, labels, max_order=i)["bleu"] for i in range(1, 5)}


def evaluate(trainer, eval_loaders: Dict[str, Iterable[dict]], lang_code_to_id: Dict[str, int],
             batch_decode: Callable[[Iterable[Sequence[int]]], List[str]], *, predict_with_generate: bool = True,
             max_length: int = 64, num_beams: int = 4, word_tokenize: Callable[[str], List[str]] = simple_word_tokenize) -> Dict[str, object]:
    """The evaluation block of the training loop (main.py:791-846).  `eval_loaders` maps a language code ("en_XX", ...) to an
    iterable of batches (the dicts `collate_fn` builds: pixel_values, input_ids, attention_mask, decoder_input_ids).
    Returns {"loss": mean eval loss over all batches, "<lang>": {"BLEU-1"..}} like `eval_metrics` (main.py:838-841)."""
    losses: List[float] = []
    out: Dict[str, object] = {}
    model = trainer.model
    for lang, loader in eval_loaders.items():
        preds, labels = [], []
        for batch in loader:
            losses.append(float(trainer.eval_step(batch)["loss"]))  # main.py:812
            if predict_with_generate:
                gen = model.generate(batch["pixel_values"], max_length=max_length, num_beams=num_beams,
                                     decoder_start_token_id=lang_code_to_id[lang])  # main.py:723-729, 820
                preds.extend(np.asarray(gen.sequences.cpu()).reshape(-1, max_length))
                lb = batch["input_ids"]
                labels.extend(np.asarray(lb.cpu() if hasattr(lb, "cpu") else lb).reshape(-1, np.asarray(lb).shape[-1]))
        if predict_with_generate:
            out[lang] = compute_metrics(preds, labels, batch_decode, word_tokenize)
    out["loss"] = float(np.mean(losses)) if losses else float("nan")
    return out


def vocabulary_shortlist(id_arrays, always=()) -> np.ndarray:
    """The sorted unique int32 token ids that occur in an iterable of label arrays (any shape, e.g. the `input_ids` of the
    training captions), plus `always` (EOS, the language ids ...): the `allowed_token_ids` of `generate` / `generate_languages`
    for a model that only ever has to write what its captions contain."""
    parts = [np.asarray(list(always), dtype=np.int64).reshape(-1)]
    for a in id_arrays:
        a = np.asarray(a.cpu() if hasattr(a, "cpu") else a)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"vocabulary_shortlist: token ids must be integers, got dtype {a.dtype}")
        parts.append(a.reshape(-1).astype(np.int64))
    ids = np.unique(np.concatenate(parts))
    if ids.size and (ids[0] < 0 or ids[-1] > np.iinfo(np.int32).max):
        raise ValueError(f"vocabulary_shortlist: token ids out of range: min {int(ids[0])}, max {int(ids[-1])}")
    return ids.astype(np.int32)


def generate_languages(model, pixel_values, lang_ids: Dict[str, int], *, via: str = "forced_bos", max_length: int = 64,
                       num_beams: int = 4, allowed_token_ids=None, num_return_sequences=None) -> Dict[str, np.ndarray]:
    """Captions of the same images in every language of `lang_ids` ({"en_XX": id, ...}) from ONE `generate` call: the language
    ids go in as a sequence, the images are encoded once and all languages share one decode chain; the result per language is
    that of its own call (`evaluation.py:80-94` calls generate once per language).  `via` names the argument that selects the
    language: "forced_bos" (`forced_bos_token_id`) or "decoder_start" (`decoder_start_token_id`, main.py:820).
    `allowed_token_ids`: the vocabulary shortlist of `generate`, shared by all languages (see `vocabulary_shortlist`).
    `num_return_sequences=N`: the N best beam hypotheses per image and language, best first (row image * N + j), see `generate`.
    Returns {language: int32 ids [batch, max_length]} ([batch * N, max_length] with N).  `evaluate()` keeps one call per language: its loaders carry different
    images per language."""
    arg = {"forced_bos": "forced_bos_token_id", "decoder_start": "decoder_start_token_id"}.get(via)
    if arg is None:
        raise ValueError(f"via={via!r}: expected 'forced_bos' or 'decoder_start'")
    langs = list(lang_ids)
    gen = model.generate(pixel_values, max_length=max_length, num_beams=num_beams, allowed_token_ids=allowed_token_ids,
                         num_return_sequences=num_return_sequences, **{arg: [int(lang_ids[l]) for l in langs]})
    seq = np.asarray(gen.sequences.cpu())
    return {l: seq[g] for g, l in enumerate(langs)}


def sequences_to_score_inputs(sequences, eos_token_id: int, pad_token_id: int):
    """What `model.score` needs to re-score the rows `generate` returned: sequences [R, L] (start token first) ->
    (decoder_input_ids = seq[:, :-1], labels = seq[:, 1:], attention_mask) as int64 / int64 / int32 numpy arrays [R, L - 1].  The
    mask covers each row of labels up to and including its first EOS — the positions `generate` summed its `scores` over — or the
    whole row when it holds none (a caption cut off at max_length).
    Greedy search and sampling write the EOS they end a row with as PAD (generate's loop: "EOS itself -> PAD"), so a row WITHOUT an
    EOS that holds a PAD ended at its first PAD: the mask covers the row up to and including that position and the label there is
    EOS, the token that was drawn.  (A PAD drawn as an ordinary token in the middle of a sampled caption cannot be told from that;
    with a trained model it has no probability to speak of.)  Behind the mask the labels stay what `generate` left there."""
    seq = np.asarray(sequences.cpu() if hasattr(sequences, "cpu") else sequences)
    if seq.ndim != 2 or seq.shape[1] < 2 or not np.issubdtype(seq.dtype, np.integer):
        raise ValueError(f"sequences_to_score_inputs: integer sequences [rows, length >= 2], got {seq.dtype} {seq.shape}")
    seq = seq.astype(np.int64)
    dec_in, labels = seq[:, :-1].copy(), seq[:, 1:].copy()
    is_eos, is_pad = labels == int(eos_token_id), labels == int(pad_token_id)
    ended_as_pad = ~is_eos.any(1) & is_pad.any(1)
    r = np.nonzero(ended_as_pad)[0]
    labels[r, is_pad[r].argmax(1)] = int(eos_token_id)
    is_eos = labels == int(eos_token_id)
    first = np.where(is_eos.any(1), is_eos.argmax(1), labels.shape[1] - 1)
    mask = (np.arange(labels.shape[1])[None, :] <= first[:, None]).astype(np.int32)
    return dec_in, labels, mask


def rerank_scores(log_likelihood, num_tokens, n_per_image: int, length_penalty: float = 1.0):
    """The arithmetic of `rerank` on host arrays: scores [images, n] = ll / num_tokens ** length_penalty (a row without tokens
    scores -inf) and, per image, the index of the best candidate (the first of equals)."""
    ll = np.asarray(log_likelihood, dtype=np.float64).reshape(-1)
    nt = np.asarray(num_tokens, dtype=np.float64).reshape(-1)
    n = int(n_per_image)
    if n < 1 or ll.shape != nt.shape or ll.size % n:
        raise ValueError(f"rerank: {ll.size} scored rows do not divide into groups of {n_per_image}")
    with np.errstate(divide="ignore", invalid="ignore"):
        scores = np.where(nt > 0, ll / np.power(np.maximum(nt, 1.0), float(length_penalty)), -np.inf).reshape(-1, n)
    return scores.argmax(1).astype(np.int64), scores.astype(np.float32)


def rerank(model, pixel_values, sequences, n_per_image: int, length_penalty: float = 1.0):
    """Rerank the n_per_image candidates `generate(num_return_sequences=n)` returned per image (rows image-major: image * n + j) by
    their teacher-forced log-likelihood, one `model.score` pass in which an image is encoded once for all its candidates.
    Returns (best int64 [images]: the index j of the best candidate, scores fp32 [images, n] = ll / num_tokens ** length_penalty)."""
    mc = model.config.mbart_config
    dec_in, labels, mask = sequences_to_score_inputs(sequences, mc.eos_token_id, mc.pad_token_id)
    out = model.score(pixel_values, labels, mask, decoder_input_ids=dec_in, candidates_per_image=int(n_per_image))
    return rerank_scores(out["log_likelihood"].cpu().numpy(), out["num_tokens"].cpu().numpy(), n_per_image, length_penalty)


def scst_advantages(rewards, n_per_image: int, baseline="mean_others"):
    """Self-critical advantages of `n_per_image` sampled captions per image: rewards [images * n] (image-major: row image * n + j) ->
    float32 advantages [images * n] = reward - baseline.  baseline: "mean_others" — the mean reward of the image's OTHER n - 1 samples
    (unbiased: a sample's baseline does not depend on the sample; n = 1 has no others: ValueError) —, "mean" — the image's mean
    reward —, or an array [images] of explicit baselines, e.g. the reward of each image's greedy caption.  Pure host function."""
    r = np.asarray(rewards, dtype=np.float64).reshape(-1)
    n = int(n_per_image)
    if n < 1 or r.size % n:
        raise ValueError(f"scst_advantages: {r.size} rewards do not divide into groups of {n_per_image}")
    g = r.reshape(-1, n)
    if isinstance(baseline, str):
        if baseline == "mean_others":
            if n == 1:
                raise ValueError("scst_advantages: baseline='mean_others' needs n_per_image >= 2 (one sample has no others)")
            b = (g.sum(1, keepdims=True) - g) / (n - 1)
        elif baseline == "mean":
            b = g.mean(1, keepdims=True)
        else:
            raise ValueError(f"scst_advantages: baseline={baseline!r}: expected 'mean_others', 'mean' or an array [images]")
    else:
        b = np.asarray(baseline, dtype=np.float64)
        if b.shape != (g.shape[0],):
            raise ValueError(f"scst_advantages: an explicit baseline has one entry per image [{g.shape[0]}], got {list(b.shape)}")
        b = b[:, None]
    return (g - b).reshape(-1).astype(np.float32)


def self_critical_batch(model, pixel_values, reward_fn, n_samples: int, prng_key, max_length: int = 64, baseline="mean_others",
                        **generate_kwargs):
    """One batch of self-critical sequence training (the policy-gradient loss -(r - b) log p(sample)):
      1. `model.generate(pixel_values, do_sample=True, num_return_sequences=n_samples, prng_key=prng_key, max_length=max_length,
         num_beams=1, **generate_kwargs)` draws n_samples captions per image in one chain (rows image-major),
      2. `sequences_to_score_inputs` turns them into decoder inputs, labels and the mask up to each caption's end,
      3. `reward_fn(sequences)` — int ndarray [R, L], the rows as `generate` returned them — gives rewards [R]: the caller's metric on
         the caller's terms (nothing is tokenised or decoded here),
      4. `scst_advantages(rewards, n_samples, baseline)`.
    Returns (batch, rewards float32 [R]); `batch` goes to `Trainer.train_step` as it is: pixel_values, input_ids (the labels),
    attention_mask, decoder_input_ids, captions_per_image = n_samples, loss_weights.
    The sign.  The train step MINIMISES sum_r w[r] sum_t m[r,t] nll[r,t] / sum m with nll = -log p.  The self-critical loss
    -(r - b) log p(sample) is (r - b) * nll, so loss_weights = +advantage: a sample that beat its baseline has a positive weight on
    its nll, descent lowers that nll — its likelihood rises — and a sample below its baseline has a negative weight and is pushed
    away from.  (-advantage is the coefficient of log p, not of the per-token loss the weights multiply.)"""
    n = int(n_samples)
    generate_kwargs.setdefault("num_beams", 1)  # sampling is one beam per draw (a config default of several beams would refuse do_sample)
    gen = model.generate(pixel_values, do_sample=True, num_return_sequences=n, prng_key=prng_key, max_length=max_length, **generate_kwargs)
    seq = gen.sequences
    seq = np.asarray(seq.cpu() if hasattr(seq, "cpu") else seq)
    mc = model.config.mbart_config
    dec_in, labels, mask = sequences_to_score_inputs(seq, mc.eos_token_id, mc.pad_token_id)
    rewards = np.asarray(reward_fn(seq), dtype=np.float32).reshape(-1)
    if rewards.shape != (seq.shape[0],):
        raise ValueError(f"self_critical_batch: reward_fn returned {rewards.size} rewards for {seq.shape[0]} sampled captions")
    if not np.isfinite(rewards).all():
        raise ValueError("self_critical_batch: reward_fn returned non-finite rewards")
    batch = {"pixel_values": pixel_values, "input_ids": labels, "attention_mask": mask, "decoder_input_ids": dec_in,
             "captions_per_image": n, "loss_weights": scst_advantages(rewards, n, baseline)}
    return batch, rewards
