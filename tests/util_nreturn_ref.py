"""References for generate(num_return_sequences=N) (tests/test_generate_nreturn_{cpu,gpu}.py, tests/test_sample_keyed_gpu.py): the beam
loop of oracle/generation_ref.py returning ALL K final hypotheses, a stepper that records each step's logits, the sampling loop with
the fp64 log-likelihood of every caption as drawn, the per-draw key schedule, and the threefry counters of a grouped row.  A helper
module, not a conftest; numpy and the oracle only."""
from __future__ import annotations

import numpy as np

from oracle import generation_ref as G

NEG = G.NEG


# ------------------------------------------------------------------------------------------------ beam search, all K hypotheses
def beam_search_all(stepper, batch_size, num_beams, start_token, max_length, pad_token_id, eos_token_id, length_penalty, early_stopping, procs):
    """gen:665-990 as `generation_ref.beam_search` states it, step for step, but returning gen:980-984's whole sorted state:
    (sequences [B, K, max_length], scores [B, K], steps) — ascending, best last, so `[..., -1]` is `beam_search`'s result and column
    K-1-j the j-th best.  Slots that never held a finished hypothesis are PAD rows with the score NEG."""
    B, K = batch_size, num_beams
    sequences = np.full((B, K, max_length), pad_token_id, dtype=np.int32)
    running_sequences = sequences.copy()
    running_sequences[:, :, 0] = start_token
    finished = np.zeros((B, K), dtype=bool)
    running_scores = np.tile(np.array([0.0] + [NEG] * (K - 1), dtype=np.float32), (B, 1))
    scores = np.full((B, K), NEG, dtype=np.float32)
    cur_len, steps = 1, 0
    lp = np.float32(length_penalty)
    rows = np.arange(B)[:, None]

    def cond():  # gen:798-820
        best_running = running_scores[:, -1:] / np.float32(float(max_length) ** float(length_penalty))
        worst_finished = np.where(finished, scores.min(axis=1, keepdims=True), NEG)
        return cur_len < max_length and not (bool(finished.all()) and early_stopping) and bool(np.all(worst_finished < best_running))

    first = True
    while first or cond():
        first = False
        logits = stepper.step(running_sequences[:, :, cur_len - 1].reshape(B * K)).astype(np.float32).reshape(B, K, -1)
        V = logits.shape[-1]
        steps += 1
        logp = G._apply(procs, running_sequences.reshape(B * K, -1), G.log_softmax(logits).reshape(B * K, V), cur_len).reshape(B, K, V)
        topk_lp, topk_idx = G.top_k((logp + running_scores[:, :, None]).reshape(B, K * V), 2 * K)  # gen:857-873
        topk_beam = topk_idx // V
        topk_seq = running_sequences[rows, topk_beam].copy()
        topk_seq[:, :, cur_len] = (topk_idx % V).astype(np.int32)
        just_fin = topk_seq[:, :, cur_len] == eos_token_id
        topk_lp = topk_lp + just_fin.astype(np.float32) * NEG  # gen:890
        nxt = G.top_k(topk_lp, K)[1][:, ::-1]
        next_running_sequences, next_running_scores = topk_seq[rows, nxt], topk_lp[rows, nxt]
        topk_lp = topk_lp / (np.float32(cur_len) ** lp)  # gen:910
        full = np.broadcast_to(finished.all(axis=-1, keepdims=True), just_fin.shape) & early_stopping
        topk_lp = topk_lp + ((~just_fin) | full).astype(np.float32) * NEG  # gen:918-919
        merged_scores = np.concatenate([scores, topk_lp], axis=1)
        mi = G.top_k(merged_scores, K)[1][:, ::-1]  # gen:932-934
        sequences = np.concatenate([sequences, topk_seq], axis=1)[rows, mi]
        finished = np.concatenate([finished, just_fin], axis=1)[rows, mi]
        scores = merged_scores[rows, mi]
        stepper.reorder((np.arange(B)[:, None] * K + topk_beam[rows, nxt]).reshape(-1))  # gen:945-953
        running_sequences, running_scores = next_running_sequences, next_running_scores.astype(np.float32)
        cur_len += 1
    any_fin = finished.any(axis=1)  # gen:980-984
    return (np.where(any_fin[:, None, None], sequences, running_sequences), np.where(any_fin[:, None], scores, running_scores), steps)


def n_best(all_seq, all_scores, n):
    """rows image * n + j of generate(num_beams=K, num_return_sequences=n): column K-1-j of the sorted state"""
    B, K, L = all_seq.shape
    return all_seq[:, ::-1][:, :n].reshape(B * n, L), all_scores[:, ::-1][:, :n].reshape(B * n)


# ------------------------------------------------------------------------------------------------ recorded logits
class RecordingStepper:
    """wraps a stepper (oracle.generation_ref.ModelStepper, ScriptedStepper): `logits[t]` is what step t returned, float32 [R, V]"""

    def __init__(self, stepper):
        self.inner, self.logits = stepper, []

    def step(self, tokens):
        out = np.asarray(self.inner.step(tokens), dtype=np.float32)
        self.logits.append(out.copy())
        return out

    def reorder(self, src_rows):
        self.inner.reorder(src_rows)


# ------------------------------------------------------------------------------------------------ sampling with log-likelihoods
def log_prob_fp64(v, tok):
    """log softmax(v)[tok] over the finite entries of each row of v, in float64"""
    v = np.asarray(v, np.float64)
    M = v.max(axis=-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        s = np.where(np.isfinite(v), np.exp(v - M), 0.0).sum(axis=-1)
    return v[np.arange(v.shape[0]), tok] - M[:, 0] - np.log(s)


def sample_scored(stepper, batch_size, start_token, max_length, pad_token_id, eos_token_id, key, procs, warpers, from_processed=False):
    """`generation_ref.sample` (gen:537-663), the same loop with the same draws, which also returns the float64 log-likelihood of every
    caption as drawn: the sum over the steps a row was not yet finished at — its EOS draw included — of log p(drawn token) under the
    distribution the draw was made from (the raw logits, or the processed and warped ones).  A forced token is a point mass: 0.
    Returns (sequences, scores float64 [B], steps run)."""
    rec = stepper if isinstance(stepper, RecordingStepper) else RecordingStepper(stepper)
    sequences = np.full((batch_size, max_length), pad_token_id, dtype=np.int32)
    sequences[:, 0] = start_token
    finished = np.zeros(batch_size, dtype=bool)
    running = sequences[:, 0].copy()
    scores = np.zeros(batch_size, np.float64)
    cur_len = 1
    key = np.asarray(key, dtype=np.uint32)
    while not (cur_len == max_length or finished.all()):
        k, key = G.prng_split(key)
        raw = rec.step(running).astype(np.float32)
        logits = G._apply(procs, sequences, raw, cur_len)
        for w in warpers:
            logits = w(sequences, logits, cur_len)
        dist = logits if from_processed else raw
        nxt = G.categorical(k, dist)
        scores += np.where(finished, 0.0, log_prob_fp64(dist, nxt))
        finished = finished | (nxt == eos_token_id)
        nxt = np.where(finished, pad_token_id, nxt).astype(np.int32)
        sequences[:, cur_len] = nxt
        running = nxt
        cur_len += 1
    return sequences, scores, cur_len - 1


# ------------------------------------------------------------------------------------------------ keys and counters
def draw_keys(prng_key, n):
    """the keys of the n draws of generate(do_sample=True, num_return_sequences=n, prng_key=prng_key): jax.random.split(key, n)"""
    key = np.asarray(prng_key)
    key = key.astype(np.uint32) if key.shape == (2,) else G.prng_key(int(prng_key))
    return G.prng_split(key, n)


def key_schedule(keys, max_length):
    """uint32 [max_length][n][2]: the key the step at cur_len of the `sample` loop started from keys[n] draws with (row 0 unused, zeros),
    by walking the oracle's split chain per draw"""
    out = np.zeros((max_length, len(keys), 2), np.uint32)
    for n, key in enumerate(keys):
        for cur_len in range(1, max_length):
            k, key = G.prng_split(key)
            out[cur_len, n] = k
    return out


def counters_of_rows(rows, V):
    """(c0, c1, word) per element of an [rows][V] array as jax.random.bits lays its threefry counters out: iota(rows * V) padded to an
    even count with a zero, split in halves; element e < h is word 0 of the pair (e, e + h), element e >= h word 1 of (e - h, e)"""
    n = rows * V
    h = (n + 1) // 2
    e = np.arange(n, dtype=np.int64)
    lo = e < h
    c0 = np.where(lo, e, e - h)
    c1 = np.where(lo, np.where(e + h < n, e + h, 0), e)
    return c0.reshape(rows, V), c1.reshape(rows, V), np.where(lo, 0, 1).reshape(rows, V)


def counters_of_grouped_row(images, draws, V, row):
    """the same for row `row` = image * draws + n of a grouped [images * draws][V] launch as mic_sample_rows_keyed is specified
    (include/mic_hip.h): element e = image * V + i of n_total = images * V counters — computed from the row's own indices, not by
    slicing counters_of_rows"""
    image = row // draws
    n = images * V
    h = (n + 1) // 2
    e = image * V + np.arange(V, dtype=np.int64)
    lo = e < h
    return np.where(lo, e, e - h), np.where(lo, np.where(e + h < n, e + h, 0), e), np.where(lo, 0, 1)
