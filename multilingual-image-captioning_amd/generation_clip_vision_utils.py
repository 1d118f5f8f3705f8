"""`.generate()` — greedy and beam search with the reference's semantics
(`models/flax_clip_vision_mbart/generation_clip_vision_utils.py:128-336, 368-420, 422-535, 665-990`), driven from the
host as a fixed sequence of HIP launches per step:

    decoder step (KV-cached)  ->  tied head GEMM  ->  mic_row_lse_topk (log-softmax + processors + running score +
    index-stable top-2K)  ->  mic_beam_step (all of gen:872-966 for one step, on device)

Differences in mechanism, not in results: cross-attention K/V are projected once (the reference re-projects every
step), and the self-attention cache is never gathered by beam (gen:945-953) — a slot-ownership table is updated
instead.  `_sample` (gen:537-663): the categorical draw is `mic_sample_rows` (Gumbel-argmax with jax's
threefry2x32 stream); by default it draws from the RAW logits exactly like the reference does (its processed/warped logits
are computed and dropped, gen:620-627); `sample_from_processed_logits=True` applies processors, temperature, top-k and
top-p (`mic_warp_thresholds`).

Decode plans and launch-free decoder steps: a decoder step is ~140 kernel launches whose arguments depend only on (batch,
beams, max_length, processors, step index) — never on the data.  Greedy and beam search keep a `_DecodePlan` per such
configuration: its device state (sequences, scores, KV cache, slot table ...) lives at fixed addresses and is re-initialised in
place per call (no 3 GB cache allocation + zero fill per generate call).  With `MIC_DECODE_GRAPHS=1` the second call of a plan
additionally captures step t of the loop into a hipGraph (one graph per step index: the cache slot, the valid length and the
processor switches are baked-in launch arguments) and from then on a step is ONE graph launch.  The host never waits inside
the loop except for a stop-flag poll every 8 steps (`lax.while_loop` in the reference has no host in it either, gen:976).
One driver, `_run_chain`, owns that loop for greedy search, beam search (sliced, unsliced, grouped) and grouped sampling: a strategy
hands it the launches of one step and its host stop test.
MEASURED (MI355X, ROCm 7.2, with a host-side probe that is no longer in the tree, ms per decoder step, graphs vs eager): batch 256 x 4 beams 2.71 vs
2.70 (GPU-bound either way), batch 32: 1.61 vs 1.62, batch 4: 1.47 vs 1.57 — a replayed 140-node graph costs what 140
back-to-back launches cost: the ~10 us per dependent kernel are the kernels' own durations (a chain of first-tile miss, K loop,
reduction and epilogue), not launch overhead, so the graphs are correct (tests) but buy nothing for a single chain and stay
opt-in there; fewer, fatter kernels per step are what would move small-batch latency.  A beam search cut into image slices
(MIC_DECODE_SLICES) uses the graphs to run the slices' chains as parallel branches.

Vocabulary shortlist (`generate(allowed_token_ids=A)`): the head GEMM runs over the len(A) gathered rows of the tied embedding
(`engine.Shortlist`), the top-k kernels over those columns with a token map (`mic_row_lse_topk_mapped`, `mic_row_topk_tiles_mapped`):
the candidates leave as vocabulary ids, so `mic_beam_step` / `mic_greedy_step` and the embedding lookup of the next step see no
difference, and the step has the same number of launches.  A decode plan is keyed by the shortlist's identity and keeps the object
alive: captured steps hold its tensors' addresses, the column count and the EOS column.

Several captions per image (`generate(num_return_sequences=N)`): sampling runs its N draws per image as one chain of images x N rows from
a decode plan (`_sample_group`: `mic_sample_rows_keyed` reads the N keys of the step from a device table and adds each draw's
log-probability to the row's score; the step body, `_sample_step_fn`, is the one `_sample` runs with `mic_sample_rows` and a host
key); beam search returns the N best of the K hypotheses it ends with (`_beam_result` / `_n_best`: gen:987-990 at N columns, N = 1
being the plain call).  None or 1 leaves `_sample` the mechanism it was.
"""
from __future__ import annotations

import operator
from typing import Optional

import torch

from . import ops

NEG = -1.0e7
_POLL = 8          # decoder steps between two looks at the device-side stop flag
_MAX_PLANS = 2     # decode plans kept per model (each owns a KV cache: 24 x rows x max_length x d_model elements)
_MAX_SHORTLISTS = 4  # vocabulary shortlists kept per model (each owns len(A) gathered embedding rows)
_AUTO_SLICES = 1   # MIC_DECODE_SLICES=auto


# Captured graphs of dropped plans are never destroyed while the process lives.  On this stack (ROCm 7.2) destroying an instantiated
# graph with parallel branches — the sliced beam search — breaks the NEXT multi-branch graph: its replay dies inside
# hip::Graph::UpdateStreams (hipGraphLaunch -> GraphExec::Run; rocgdb backtrace in profiles/README.md).  As long as models lingered in
# reference cycles the graphs happened to outlive every later replay; now that a dropped model frees its device state at once, the
# graph objects (host-side nodes, no device memory of their own: nothing is allocated inside a capture) are parked here instead.
_RETIRED_GRAPHS = []


def _id_sequence(name: str, value):
    """None for a scalar (or None); the list of ints for a list / tuple / 1-D integer array"""
    import numpy as np

    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    if isinstance(value, np.ndarray):
        if value.ndim == 0:
            return None
        if value.ndim != 1 or not np.issubdtype(value.dtype, np.integer):
            raise ValueError(f"`{name}`: a sequence of language ids must be a 1-D integer array, got shape {value.shape} dtype {value.dtype}")
        value = value.tolist()
    elif not isinstance(value, (list, tuple)):
        return None
    if len(value) == 0:
        raise ValueError(f"`{name}`: empty sequence of language ids")
    for v in value:
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"`{name}`: language ids must be integers, got {v!r}")
    return [int(v) for v in value]


def normalize_language_ids(decoder_start_token_id=None, forced_bos_token_id=None):
    """`generate()`'s language arguments -> (G, bos_ids, start_ids, grouped).

    Either argument may be a scalar (or None: the config's default applies later) or a sequence of G >= 1 ints — list, tuple,
    1-D numpy / torch integer array.  A sequence selects the grouped call (G separate searches on the same images) whatever its
    length: the type decides.  Two sequences must have the same length; a scalar beside a sequence is broadcast.  bos_ids /
    start_ids are lists of G ints, or None where the argument was None.  Scalars: G = 1, grouped False, one-element lists."""
    seqs = {"decoder_start_token_id": _id_sequence("decoder_start_token_id", decoder_start_token_id),
            "forced_bos_token_id": _id_sequence("forced_bos_token_id", forced_bos_token_id)}
    given = [v for v in seqs.values() if v is not None]
    if len(given) == 2 and len(given[0]) != len(given[1]):
        raise ValueError(f"`decoder_start_token_id` lists {len(given[0])} languages, `forced_bos_token_id` {len(given[1])}")
    if not given:  # today's scalar call: the values pass through untouched
        return 1, (None if forced_bos_token_id is None else [forced_bos_token_id]), \
            (None if decoder_start_token_id is None else [decoder_start_token_id]), False
    G = len(given[0])
    out = []
    for name, raw in (("forced_bos_token_id", forced_bos_token_id), ("decoder_start_token_id", decoder_start_token_id)):
        if seqs[name] is not None:
            out.append(seqs[name])
        elif raw is None:
            out.append(None)
        else:
            try:
                out.append([operator.index(raw.item() if hasattr(raw, "item") else raw)] * G)
            except (TypeError, ValueError):
                raise ValueError(f"`{name}`: expected an integer or a sequence of integers, got {raw!r}") from None
    return G, out[0], out[1], True


def normalize_allowed_token_ids(allowed_token_ids, vocab_size: int, *, eos_token_id=None, forced_bos_token_id=None,
                                forced_eos_token_id=None, language_bos_ids=None, num_beams: int = 1, do_sample: bool = False):
    """`generate(allowed_token_ids=A)` -> A as a sorted, duplicate-free int32 numpy array (sorted: the head's compact column order is
    then vocabulary order, so top-k ties break by ascending token id exactly as over the whole vocabulary).

    A is a 1-D integer sequence (list, tuple, numpy or torch).  ValueError for an empty, non-integer or non-1-D A, ids outside
    [0, vocab_size), and for anything the search must be able to emit but could not: `eos_token_id`, the scalar `forced_bos_token_id` /
    `forced_eos_token_id` in force for the call, every entry of `language_bos_ids` (the per-language BOS ids of a grouped call) — pass
    None for what is not in force — and len(A) < 2 * num_beams for a beam search (top-k refuses k > columns).  Start ids are inputs and
    PAD is written by the bookkeeping: neither has to be in A.  Sampling draws noise per vocabulary column: NotImplementedError."""
    import numpy as np

    a = allowed_token_ids
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    if isinstance(a, (list, tuple)):
        for v in a:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"`allowed_token_ids`: token ids must be integers, got {v!r}")
        a = np.asarray(a, dtype=np.int64)
    if not isinstance(a, np.ndarray):
        raise ValueError(f"`allowed_token_ids`: expected a 1-D sequence of integers, got {type(allowed_token_ids).__name__}")
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"`allowed_token_ids` must be a 1-D integer array, got shape {a.shape} dtype {a.dtype}")
    if a.size == 0:
        raise ValueError("`allowed_token_ids` is empty")
    if int(a.min()) < 0 or int(a.max()) >= vocab_size:
        raise ValueError(f"`allowed_token_ids` holds ids outside the vocabulary [0, {vocab_size}): min {int(a.min())}, max {int(a.max())}")
    ids = np.unique(a).astype(np.int32)  # sorted
    if do_sample:
        raise NotImplementedError("do_sample=True with `allowed_token_ids` is not implemented: the sampling noise is indexed by vocabulary "
                                  "column; a shortlist serves greedy and beam search only")

    def member(v) -> bool:
        i = int(np.searchsorted(ids, v))
        return i < ids.size and int(ids[i]) == int(v)

    for name, v in (("eos_token_id", eos_token_id), ("forced_bos_token_id", forced_bos_token_id), ("forced_eos_token_id", forced_eos_token_id)):
        if v is not None and not member(v):
            raise ValueError(f"`{name}`={int(v)} is not in `allowed_token_ids`: the search has to be able to emit it")
    for v in language_bos_ids or ():
        if not member(v):
            raise ValueError(f"the language id {int(v)} (`forced_bos_token_id`) is not in `allowed_token_ids`")
    if num_beams > 1 and ids.size < 2 * num_beams:
        raise ValueError(f"`allowed_token_ids` has {ids.size} distinct ids: beam search with num_beams={num_beams} ranks 2 * num_beams = "
                         f"{2 * num_beams} candidates per row")
    return ids


def normalize_num_return_sequences(num_return_sequences, *, do_sample: bool, num_beams: int) -> int:
    """`generate(num_return_sequences=N)` -> N (1 for None).  What `generate` refuses without the argument keeps its error and message
    and comes first (beam sampling, gen:336; num_beams > 32).  ValueError: N not an integer (a bool is not one) or < 1, N > 1 with
    greedy search (one image has one greedy caption), N > num_beams for a beam search (it ends with num_beams hypotheses per image)."""
    if num_return_sequences is None:
        return 1
    if do_sample and num_beams > 1:
        raise NotImplementedError("`Beam sampling is currently not implemented.")  # gen:336
    if not do_sample and 2 * num_beams > 64:
        raise NotImplementedError("num_beams > 32 needs a wider per-row top-k than this build ships (k = 2*num_beams <= 64)")
    try:
        if isinstance(num_return_sequences, bool):
            raise TypeError
        N = operator.index(num_return_sequences)
    except TypeError:
        raise ValueError(f"`num_return_sequences` must be an integer >= 1, got {num_return_sequences!r}") from None
    if N < 1:
        raise ValueError(f"`num_return_sequences` must be an integer >= 1, got {N}")
    if N > 1 and not do_sample and num_beams == 1:
        raise ValueError(f"num_return_sequences={N} with greedy search: one image has one greedy caption; use do_sample=True or num_beams >= {N}")
    if not do_sample and N > num_beams:
        raise ValueError(f"num_return_sequences={N} exceeds num_beams={num_beams}: a beam search ends with num_beams hypotheses per image")
    return N


class _DecodePlan:
    """Fixed-address device state of one generate configuration + its captured decoder steps."""

    def __init__(self):
        self.shortlist = None  # generate(allowed_token_ids=...): the engine.Shortlist whose tensors the captured steps point into
        self.t = {}          # name -> persistent tensor
        self.graphs = {}     # cur_len -> torch.cuda.CUDAGraph
        self.calls = 0
        self.stream = None   # capture stream
        self.subs = []       # beam search: one sub-plan (state tensors + KV cache) per image slice
        self.streams = []    # ... and the streams their chains run on
        self.graph_events = {}  # cur_len -> the fork / join events recorded while that step was captured (kept as long as the graph)
        self._events_now = []

    def __del__(self):
        # see _RETIRED_GRAPHS: multi-branch graphs (a sliced beam search: `streams` is non-empty) and the events recorded into them
        # outlive the plan; single-chain graphs are destroyed with it (a server cycling through plans must not accumulate them)
        try:
            if self.streams:
                _RETIRED_GRAPHS.extend((g, self.graph_events.get(k)) for k, g in self.graphs.items())
                if _RETIRED_GRAPHS and len(_RETIRED_GRAPHS) % 256 == 0:
                    import sys

                    print(f"[mic_amd.generate] {len(_RETIRED_GRAPHS)} retired multi-branch decode graphs are parked (ROCm 7.2 workaround)", file=sys.stderr)
            self.graphs.clear()
        except Exception:  # interpreter shutdown
            pass

    def new_event(self) -> "torch.cuda.Event":
        """an event for the fork / join of the slices' chains; the ones recorded inside a capture are kept as long as the graph (a
        precaution: the capture turns their records into dependencies of the graph's nodes)"""
        ev = torch.cuda.Event()
        self._events_now.append(ev)
        return ev

    def run_step(self, cur_len: int, fn, use_graphs: bool):
        """fn() issues the launches of decoder step `cur_len` on the current stream.  First call of a plan: eager.  Later calls:
        replay the step's graph, capturing it the first time (capture executes nothing; the replay does)."""
        if not use_graphs or self.calls == 0:
            self._events_now = []
            fn()
            self._events_now = []
            return
        g = self.graphs.get(cur_len)
        if g is None:
            if self.stream is None:
                self.stream = torch.cuda.Stream()
            g = torch.cuda.CUDAGraph()
            self._events_now = []
            with torch.cuda.stream(self.stream):
                g.capture_begin(capture_error_mode="thread_local")
                try:
                    fn()
                finally:
                    g.capture_end()
            self.graphs[cur_len] = g
            self.graph_events[cur_len], self._events_now = self._events_now, []
        g.replay()


def _graphs_enabled(dev, slices: int = 1) -> bool:
    """per-step hipGraphs: opt-in for a single chain (a replayed chain costs what the eager launches cost), ON for a sliced beam
    search — there the graph is what makes the slices' chains parallel branches of one launch (issuing them eagerly would cost
    the host `slices` x 1.4 ms per step); MIC_DECODE_GRAPHS=0|1 forces either"""
    import os

    want = os.environ.get("MIC_DECODE_GRAPHS", "auto")
    if dev.type != "cuda" or want == "0":
        return False
    return want == "1" or slices > 1


def _run_chain(plan: _DecodePlan, step, max_length: int, stopped, use_graphs: bool) -> None:
    """The decode chain of one call on `plan`: `step(cur_len)` issues the launches of decoder step cur_len = 1 .. max_length - 1 on
    the current stream; `stopped()` is the strategy's host test (one device read) that every row / every search is done.  A step
    issued after that point changes nothing — greedy and sampling: a finished row only ever receives PAD (gen:501-507, 629-642) into
    a buffer that is PAD already; beam search: mic_beam_step evaluates `beam_search_cond_fn` (gen:798-820) on the device and is a
    no-op once it said stop — so the host enqueues steps (graph replays once the plan is warm) without waiting and asks only every
    _POLL steps: in front of steps _POLL + 1, 2 * _POLL + 1, ...  Step 1 carries the call's forced-BOS id and is never captured."""
    for cur_len in range(1, max_length):
        if cur_len > 1 and (cur_len - 1) % _POLL == 0 and stopped():
            break
        plan.run_step(cur_len, lambda: step(cur_len), use_graphs and cur_len > 1)
    plan.calls += 1


class FlaxCLIPVisionMBartGenerationMixin:
    # ------------------------------------------------------------------ gen:128-336
    def generate(self, input_ids, max_length: Optional[int] = None, pad_token_id: Optional[int] = None,
                 bos_token_id: Optional[int] = None, eos_token_id: Optional[int] = None,
                 decoder_start_token_id: Optional[int] = None, do_sample: Optional[bool] = None, prng_key=None,
                 top_k: Optional[int] = None, top_p: Optional[float] = None, temperature: Optional[float] = None,
                 num_beams: Optional[int] = None, no_repeat_ngram_size: Optional[int] = None, min_length: Optional[int] = None,
                 forced_bos_token_id: Optional[int] = None, forced_eos_token_id: Optional[int] = None,
                 length_penalty: Optional[float] = None, early_stopping: Optional[bool] = None, trace: bool = True,
                 params=None, allowed_token_ids=None, num_return_sequences: Optional[int] = None, **model_kwargs):
        """`FlaxCLIPVisionGenerationMixin.generate` (gen:128-336): same arguments, defaults from `config.mbart_config`, same dispatch —
        greedy (`num_beams == 1`, no sampling), sampling (`do_sample`, one beam) or beam search; `input_ids` = pixel values.
        Limits of this build (the reference has none of the first two; the third is the reference's own): `num_beams <= 32` — the fused
        per-row top-2K kernel keeps k = 2 * num_beams <= 64 candidates per row, a wider search raises NotImplementedError (the reference's
        evaluation runs num_beams = 4, evaluation.py:80-94); `max_length <= max_position_embeddings` (XLA's gather would clamp silently,
        this raises); beam search with sampling raises NotImplementedError as upstream (gen:336).

        Several languages in one call: `forced_bos_token_id` and / or `decoder_start_token_id` may be a sequence of G >= 1 ints (list,
        tuple, 1-D numpy / torch integer array; a scalar beside a sequence is broadcast, two sequences must agree in length; a sequence of
        length 1 still takes this path).  The result is that of G separate calls on the same images, one per entry — each with its own
        stop test (gen:798-820 is `jnp.all` over the images of ONE call) — computed as one decode chain of G x the rows: the encoder runs
        once, cross-attention K/V are projected once per image, decoder row = (image * G + g) * num_beams + beam.  Returns
        `sequences [G, B, max_length]` and, for beam search, `scores [G, B]` and `out["steps"]` = a list of G step counts.  Greedy and
        beam search only (`do_sample=True` raises NotImplementedError); the search runs unsliced (MIC_DECODE_SLICES is ignored here);
        MIC_DECODE_GRAPHS=1 works as for a single chain.

        Vocabulary shortlist: `allowed_token_ids=A` (a 1-D integer sequence: list, tuple, numpy or torch; order and duplicates do not matter)
        returns what the same call returns on a model whose `final_logits_bias` is -inf outside A and unchanged inside: log-softmax
        normalised over A, top-k ties to the lower vocabulary id, `scores` accordingly, the processors and stop tests as they are.  The
        LM head then runs over len(A) gathered rows of the tied embedding instead of the whole vocabulary (gathered once per distinct A and
        kept on the model; refreshed in place when the weights move).  `eos_token_id`, a scalar forced BOS / EOS id in force, every
        per-language BOS id and, for beam search, len(A) >= 2 * num_beams are required of A (ValueError, before any device work); start ids
        and PAD need not be in it.  One set per call (the languages of a grouped call share it); `do_sample=True` raises
        NotImplementedError.  None (default): the whole vocabulary.

        Several captions per image: `num_return_sequences=N` (the argument and output layout of the PyTorch `generate`; the reference's
        Flax `generate` has none).  None or 1: every path is what it is without the argument.  Sampling (`do_sample=True`, one beam,
        N >= 2): N independent draws per image from ONE decode chain — `keys = jax.random.split(PRNGKey(prng_key), N)`, and draw n is
        what `generate(same arguments, prng_key=keys[n])` returns (float32: token ids bit for bit; both sampling modes).  Returns
        `sequences [B*N, max_length]` (row image * N + n) and `scores [B*N]`: the log-likelihood of each caption as drawn — the sum over
        its steps, the EOS draw included, of log p(token) under the distribution the draw was made from (raw logits in the reference's
        mode, the processed and warped ones with `sample_from_processed_logits=True`; a forced token adds 0).  The images are encoded
        once, cross K/V projected once per image, the state lives in a decode plan (MIC_DECODE_GRAPHS=1 replays the steps; the per-step
        keys are a device table, so a warm plan serves any `prng_key`).  Beam search (`num_beams = K`, 1 <= N <= K): the N best of the K
        hypotheses the search ends with, best first — `sequences [B*N, max_length]`, `scores [B*N]`, row image * N + j = gen:980-990 read
        at column K-1-j instead of -1 (row j = 0 is the plain call's result bit for bit; `out["steps"]` is unchanged); with a sequence
        of language ids `[G, B*N, max_length]` and `[G, B*N]`.  Slots that never held a finished hypothesis come back as they lie in
        the state: an image with fewer than N finished hypotheses returns PAD rows with the score -1e7 for the rest (an image with none
        returns its running hypotheses).  ValueError, before the encoder runs: N < 1 or not an integer, N > 1 with greedy search,
        N > num_beams."""
        mc = self.config.mbart_config
        G, bos_ids, start_ids, grouped = normalize_language_ids(decoder_start_token_id, forced_bos_token_id)
        if grouped:  # resolved per language below; the scalar code in between sees "not given"
            decoder_start_token_id = forced_bos_token_id = None
        from_processed = bool(model_kwargs.pop("sample_from_processed_logits", False))  # build-only switch, see _sample
        max_length = max_length if max_length is not None else mc.max_length  # gen:205-209
        bos_token_id = bos_token_id if bos_token_id is not None else mc.bos_token_id
        pad_token_id = pad_token_id if pad_token_id is not None else mc.pad_token_id
        eos_token_id = eos_token_id if eos_token_id is not None else mc.eos_token_id
        decoder_start_token_id = decoder_start_token_id if decoder_start_token_id else mc.decoder_start_token_id  # gen:225-229
        if decoder_start_token_id is None and self.config.is_encoder_decoder and not (grouped and start_ids is not None and all(start_ids)):
            raise ValueError("`decoder_start_token_id` has to be defined for encoder-decoder generation.")  # gen:232-235
        do_sample = do_sample if do_sample is not None else mc.do_sample
        num_beams = num_beams if num_beams is not None else mc.num_beams
        if max_length < 2:
            raise ValueError(f"max_length={max_length}: generation needs room for the start token and one more")
        if max_length > mc.max_position_embeddings:
            # the learned position table has max_position_embeddings (+2 offset) rows; XLA's gather would clamp silently
            raise ValueError(f"max_length={max_length} exceeds mbart_config.max_position_embeddings={mc.max_position_embeddings}")
        lang = None
        if grouped:
            if do_sample:
                raise NotImplementedError("do_sample=True with a sequence of language ids is not implemented: several languages per call "
                                          "are served by greedy and beam search only")
            if bos_ids is None and mc.forced_bos_token_id is not None:
                bos_ids = [mc.forced_bos_token_id] * G
            lang = dict(G=G, start=[s if s else decoder_start_token_id for s in (start_ids or [None] * G)], bos=bos_ids)  # gen:225-229 per language
            for ids in (lang["start"], lang["bos"] or []):  # these index the embedding table on the device
                if any(not 0 <= v < mc.vocab_size for v in ids):
                    raise ValueError(f"language ids {ids} outside the vocabulary [0, {mc.vocab_size})")
        allowed = None
        if allowed_token_ids is not None:  # host-only checks, before the encoder runs
            allowed = normalize_allowed_token_ids(
                allowed_token_ids, mc.vocab_size, eos_token_id=eos_token_id,
                forced_bos_token_id=None if lang else (forced_bos_token_id if forced_bos_token_id is not None else mc.forced_bos_token_id),
                forced_eos_token_id=forced_eos_token_id if forced_eos_token_id is not None else mc.forced_eos_token_id,
                language_bos_ids=lang["bos"] if lang else None, num_beams=num_beams, do_sample=bool(do_sample))
        N = normalize_num_return_sequences(num_return_sequences, do_sample=bool(do_sample), num_beams=num_beams)  # host-only, before the encoder runs
        # gen:109-120: `params=` is NOT forwarded to encode (the encoder always uses self.params); the decoder uses it.
        enc = self.encode(input_ids, return_dict=True, **{k: v for k, v in model_kwargs.items()
                                                          if not (k.startswith("decoder_") or k.startswith("cross_attn"))})
        self._use_params(params)
        sl = self._shortlist(allowed) if allowed is not None else None
        ehs = enc["last_hidden_state"]
        B = ehs.shape[0]
        # processors (gen:368-420); `no_repeat_ngram_size` is accepted and ignored like in the reference
        min_length = min_length if min_length is not None else mc.min_length
        forced_bos_token_id = forced_bos_token_id if forced_bos_token_id is not None else mc.forced_bos_token_id
        forced_eos_token_id = forced_eos_token_id if forced_eos_token_id is not None else mc.forced_eos_token_id
        procs = dict(min_length=min_length if (min_length is not None and eos_token_id is not None and min_length > -1) else None,
                     forced_bos=None if lang else forced_bos_token_id, forced_eos=forced_eos_token_id)  # (per-row BOS ids travel in `lang`)
        if not do_sample and num_beams == 1:
            return self._greedy_search(ehs, B, decoder_start_token_id, max_length, pad_token_id, eos_token_id, procs, lang, sl)
        elif do_sample and num_beams == 1:
            warp = dict(top_k=top_k if top_k is not None else getattr(mc, "top_k", 50),  # gen:349-356
                        top_p=top_p if top_p is not None else getattr(mc, "top_p", 1.0),
                        temperature=temperature if temperature is not None else getattr(mc, "temperature", 1.0))
            if N > 1:
                return self._sample_group(ehs, B, N, decoder_start_token_id, max_length, pad_token_id, eos_token_id, prng_key, procs, warp,
                                          from_processed)
            return self._sample(ehs, B, decoder_start_token_id, max_length, pad_token_id, eos_token_id, prng_key, procs, warp, from_processed)
        elif not do_sample and num_beams > 1:
            length_penalty = length_penalty if length_penalty is not None else mc.length_penalty  # gen:733-742
            early_stopping = early_stopping if early_stopping is not None else mc.early_stopping
            return self._beam_search(ehs, B, num_beams, decoder_start_token_id, max_length, pad_token_id, eos_token_id,
                                     length_penalty, early_stopping, procs, lang, sl, n_best=N)
        else:
            raise NotImplementedError("`Beam sampling is currently not implemented.")  # gen:336

    @staticmethod
    def _proc_args(procs, cur_len: int, max_length: int, sl=None):
        """(forced_token, suppress_eos) for this step: MinLength -> ForcedBOS -> ForcedEOS (gen:412-419); forced_token is -1
        for none and, with the vocabulary shortlist `sl`, the forced id's column in it (what the top-k over its columns counts in)."""
        forced = -1
        # FlaxMinLengthLogitsProcessor: apply_penalty = 1 - clip(cur_len - min_length, 0, 1)  =>  EOS is -inf while cur_len <= min_length
        suppress = procs["min_length"] is not None and cur_len <= procs["min_length"]
        if procs["forced_bos"] is not None and cur_len == 1:
            forced = procs["forced_bos"]
        if procs["forced_eos"] is not None and cur_len == max_length - 1:
            forced = procs["forced_eos"]
        return (sl.column(forced) if sl and forced >= 0 else forced), suppress

    # ------------------------------------------------------------------ gen:422-535
    @staticmethod
    def _plan_key(kind: str, fields: tuple, lang=None, sl=None) -> tuple:
        """the key of a decode plan: the strategy, what its launch arguments and buffer shapes depend on, then ("G", languages) for a
        grouped call and ("A", <shortlist key>) for a vocabulary shortlist"""
        return (kind,) + fields + ((("G", lang["G"]),) if lang else ()) + ((("A",) + sl.key,) if sl else ())

    def _decode_plan(self, key, build) -> _DecodePlan:
        """LRU of `_MAX_PLANS` decode plans; `build(plan)` allocates a new plan's tensors."""
        from collections import OrderedDict

        plans = self.__dict__.setdefault("_decode_plans", OrderedDict())
        plan = plans.get(key)
        if plan is None:
            while len(plans) >= _MAX_PLANS:
                plans.popitem(last=False)
            plan = plans[key] = _DecodePlan()
            build(plan)
        plans.move_to_end(key)
        return plan

    def release_decode_plans(self):
        """drop the cached decode plans (their KV caches and captured graphs)"""
        self.__dict__.pop("_decode_plans", None)

    def _shortlist(self, ids):
        """the engine.Shortlist of the sorted unique ids `ids` (normalize_allowed_token_ids): built once per distinct set, a small LRU on
        the model keyed by a digest of the ids.  A decode plan keeps the one it was built with (`_shortlist_of`)."""
        import hashlib
        from collections import OrderedDict

        from .engine import Shortlist

        key = (int(ids.size), hashlib.sha1(ids.tobytes()).hexdigest())
        cache = self.__dict__.setdefault("_shortlists", OrderedDict())
        sl = cache.get(key)
        if sl is None:
            for plan in self.__dict__.get("_decode_plans", {}).values():  # dropped from the LRU, but a plan's captured steps still point into it
                if plan.shortlist is not None and plan.shortlist.key == key:
                    sl = plan.shortlist
            if sl is None:
                sl = Shortlist(self.engine, ids, key)
            while len(cache) >= _MAX_SHORTLISTS:
                cache.popitem(last=False)
            cache[key] = sl
        cache.move_to_end(key)
        return sl

    def _shortlist_of(self, plan: _DecodePlan, eos_token_id):
        """(shortlist, columns, EOS column, token map) of a plan — (None, V, eos_token_id, None) for the whole vocabulary.  The plan's own
        shortlist object is the one its captured steps point into; its gathered rows are brought up to date with the weights here, in
        place, on the stream the steps follow on."""
        sl = plan.shortlist
        if sl is None:
            return None, self.store.V, eos_token_id, None
        sl.refresh()
        return sl, sl.Ns, (sl.column(eos_token_id) if eos_token_id is not None else eos_token_id), sl.map

    def _plan_cache(self, plan: _DecodePlan, rows: int, max_length: int) -> dict:
        """the plan's self-attention cache (modeling:249-282: static length max_length).  Not re-zeroed between calls: a step
        only reads the slots <= its own index, all written earlier in the same call."""
        if "k0" not in plan.t:
            c = self.init_cache(rows, max_length)
            for l, (k, v) in enumerate(zip(c["k"], c["v"])):
                plan.t[f"k{l}"], plan.t[f"v{l}"] = k, v
        L = self.store.L
        return {"k": [plan.t[f"k{l}"] for l in range(L)], "v": [plan.t[f"v{l}"] for l in range(L)], "cache_index": 0,
                "max_length": max_length, "rows": rows, "src_row": None, "cross": None, "row_div": 1}

    def _lang_rows(self, t, ids, images: int, beams: int, name: str):
        """plan tensor t[name] ([images * G * beams] int32) := ids[g] for row (image * G + g) * beams + beam: one small host-to-device
        copy and a broadcasting device copy"""
        G = len(ids)
        t[name].view(images, G, beams).copy_(torch.tensor(ids, dtype=torch.int32).to(self.device).view(1, G, 1).expand(images, G, beams))
        return t[name]

    def _start_tokens(self, t, first_col, next_token, start_token, lang, images: int, beams: int):
        """the start token of every row into `next_token` and into column 0 of the sequences (`first_col`, a view): the scalar
        start_token, or the language's own for the rows of a grouped call (lang = dict(G, start, bos)).  Returns the per-row
        ForcedBOS ids of such a call (t["bos_rows"]) or None."""
        if not lang:
            first_col.fill_(start_token)  # (a fill kernel: assigning a Python scalar into a device tensor is a synchronous copy)
            next_token.fill_(start_token)
            return None
        next_token.copy_(self._lang_rows(t, lang["start"], images, beams, "start_rows"))
        first_col.copy_(next_token.view(first_col.shape))
        return self._lang_rows(t, lang["bos"], images, beams, "bos_rows") if lang["bos"] is not None else None

    def _candidates(self, logits, stat, head, k: int, rows: int, top_val, top_idx, procs, cur_len: int, max_length: int, bos_rows, *,
                    raw_logits: bool = False, row_bias=None):
        """the k best continuations of every row after this step's processors, as vocabulary ids (gen:412-419, 850-873).  Greedy: k = 1 on
        the raw logits; beam search: k = 2K log-probabilities on top of the running scores (row_bias).  head = `_shortlist_of`'s tuple;
        stat: the head GEMM's per-granule partials where the decoder step returned them."""
        sl, cols, eos_col, tmap = head
        forced, suppress = self._proc_args(procs, cur_len, max_length, sl)
        if bos_rows is not None and cur_len == 1 and forced < 0:  # ForcedBOS per language (a ForcedEOS at max_length == 2 wins)
            ops.row_forced_topk(rows, k, bos_rows, top_val, top_idx, row_bias=row_bias)
        elif stat is not None and forced < 0 and k <= 16:
            # log-softmax + top-k from the head GEMM's per-granule partials: 3908 pairs and a few 64-column granules
            # per row instead of two passes over the 250 054 logits (same candidates, same order, same fp32 arithmetic)
            ops.row_topk_tiles(logits, logits.stride(0), cols, stat, k, top_val, top_idx, rows, suppress_eos=suppress, eos_token_id=eos_col,
                               raw_logits=raw_logits, row_bias=row_bias, token_map=tmap)
        else:
            ops.row_lse_topk(logits, logits.stride(0), cols, k, top_val, top_idx, rows, forced_token=forced, suppress_eos=suppress,
                             eos_token_id=eos_col, raw_logits=raw_logits, row_bias=row_bias, token_map=tmap)

    def _greedy_search(self, ehs, B, start_token, max_length, pad_token_id, eos_token_id, procs, lang=None, sl=None):
        """lang = None: B rows.  lang = dict(G, start, bos): G searches per image, row = image * G + g (n_img images below).
        sl: the engine.Shortlist of generate(allowed_token_ids=...) or None"""
        from .modeling_clip_vision_mbart import ModelOutput

        dev, st = self.device, self.store
        G = lang["G"] if lang else 1
        n_img, B = B, B * G

        def build(plan):
            t = plan.t
            t["sequences"] = torch.empty((B, max_length), dtype=torch.int32, device=dev)
            t["finished"] = torch.empty(B, dtype=torch.int32, device=dev)
            t["next_token"] = torch.empty((B,), dtype=torch.int32, device=dev)
            t["top_val"] = torch.empty((B, 1), dtype=torch.float32, device=dev)
            t["top_idx"] = torch.empty((B, 1), dtype=torch.int32, device=dev)
            t["pos_all"] = torch.arange(max_length, dtype=torch.int32, device=dev).repeat_interleave(B)
            if lang:
                t["start_rows"] = torch.empty(B, dtype=torch.int32, device=dev)
                t["bos_rows"] = torch.empty(B, dtype=torch.int32, device=dev)
            plan.shortlist = sl

        plan = self._decode_plan(self._plan_key("greedy", (B, max_length, pad_token_id, eos_token_id, procs["min_length"], procs["forced_eos"],
                                                           self.dtype), lang, sl), build)
        head = self._shortlist_of(plan, eos_token_id)
        t = plan.t
        sequences, finished, next_token, top_val, top_idx, pos_all = (t[k] for k in ("sequences", "finished", "next_token", "top_val",
                                                                                     "top_idx", "pos_all"))
        sequences.fill_(pad_token_id)  # gen:457
        finished.zero_()
        bos_rows = self._start_tokens(t, sequences[:, 0], next_token, start_token, lang, n_img, 1)
        cache = self._plan_cache(plan, B, max_length)
        self._decode_set_encoder(cache, ehs.reshape(n_img * st.S, st.d), n_img, G)

        def step(cur_len):
            with ops.pinned_stream():
                cache["cache_index"] = cur_len - 1
                logits = self._decode_step(cache, next_token, pos_all[(cur_len - 1) * B: cur_len * B], shortlist=head[0])
                self._candidates(logits, None, head, 1, B, top_val, top_idx, procs, cur_len, max_length, bos_rows, raw_logits=True)
                ops.greedy_step(B, max_length, cur_len, eos_token_id, pad_token_id, top_idx, 1, sequences, finished, next_token)

        _run_chain(plan, step, max_length, lambda: bool(finished.all().item()), _graphs_enabled(dev))  # gen:480-487: every row has finished
        if lang:
            return ModelOutput(sequences=sequences.view(n_img, G, max_length).transpose(0, 1).contiguous())
        return ModelOutput(sequences=sequences.clone())

    # ------------------------------------------------------------------ gen:537-663
    @staticmethod
    def _warp_in_force(warp, from_processed: bool):
        """(top_k, top_p, temperature) as the sampling step applies them: 0 / 1.0 / 1.0 where a warper is off, all off in the reference's
        mode (it draws from the raw logits)"""
        use_k = from_processed and warp["top_k"] not in (None, 0)
        use_p = from_processed and warp["top_p"] is not None and warp["top_p"] < 1.0
        return (warp["top_k"] if use_k else 0, float(warp["top_p"]) if use_p else 1.0,
                float(warp["temperature"] or 1.0) if from_processed else 1.0)

    def _sample_step_fn(self, t, rows: int, max_length, pad_token_id, eos_token_id, procs, warp, from_processed: bool, draw):
        """the launches of one sampling step after the decoder's: step(cur_len, logits).  t: the state tensors (sequences, finished,
        next_token, drawn and — where top-k / top-p are in force — thr, lim); warp: `_warp_in_force`'s triple;
        draw(cur_len, logits, **kw) launches the categorical draw into t["drawn"], kw being the processed mode's arguments (none in the
        reference's mode: jax.random.categorical(prng_key, model_outputs.logits[:, -1]), gen:625-627 — no processors)."""
        top_k, top_p, temp = warp
        thr, lim = t.get("thr"), t.get("lim")

        def step(cur_len, logits):
            kw = {}
            if from_processed:
                forced, suppress = self._proc_args(procs, cur_len, max_length)
                if thr is not None and forced < 0:  # gen:338-366: temperature -> top-k -> top-p, as (threshold, tie limit) per row
                    ops.warp_thresholds(logits, logits.stride(0), self.store.V, thr, lim, rows, temperature=temp, suppress_eos=suppress,
                                        eos_token_id=eos_token_id, top_k=top_k, top_p=top_p)
                kw = dict(temperature=temp, forced_token=forced, suppress_eos=suppress, eos_token_id=eos_token_id, min_keep=thr, tie_limit=lim)
            draw(cur_len, logits, **kw)
            ops.greedy_step(rows, max_length, cur_len, eos_token_id, pad_token_id, t["drawn"], 1, t["sequences"], t["finished"],
                            t["next_token"])  # gen:629-642
        return step

    def _sample(self, ehs, B, start_token, max_length, pad_token_id, eos_token_id, prng_key, procs, warp, from_processed: bool):
        # One draw per image (num_return_sequences None or 1) deliberately keeps its own mechanism: no decode plan, state allocated per
        # call, the stop test in front of every step, the host-keyed `mic_sample_rows` kernel and no `scores` in the output.  Moving it
        # onto a plan and `_run_chain` would change the memory held between calls and which kernel the sampling conformance tests
        # exercise: a behaviour decision, not a tidy-up.  It shares the step body (`_sample_step_fn`) with `_sample_group`.
        from . import prng
        from .modeling_clip_vision_mbart import ModelOutput

        dev, st = self.device, self.store
        warp = self._warp_in_force(warp, from_processed)
        t = dict(sequences=torch.full((B, max_length), pad_token_id, dtype=torch.int32, device=dev),
                 finished=torch.zeros(B, dtype=torch.int32, device=dev),
                 next_token=torch.full((B,), start_token, dtype=torch.int32, device=dev),
                 drawn=torch.empty((B, 1), dtype=torch.int32, device=dev))
        if warp[0] or warp[1] < 1.0:
            t["thr"], t["lim"] = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        t["sequences"][:, 0].fill_(start_token)  # (a fill kernel: assigning a Python scalar into a device tensor is a synchronous copy)
        key = prng.prng_key(0 if prng_key is None else prng_key)  # gen:561
        cache = self.init_cache(B, max_length)
        self._decode_set_encoder(cache, ehs.reshape(B * st.S, st.d), B, 1)
        pos = torch.zeros(B, dtype=torch.int32, device=dev)
        step = self._sample_step_fn(t, B, max_length, pad_token_id, eos_token_id, procs, warp, from_processed,
                                    lambda cur_len, logits, **kw: ops.sample_rows(logits, logits.stride(0), st.V, k, t["drawn"], B, **kw))
        for cur_len in range(1, max_length):
            if bool(t["finished"].all().item()):  # gen:596-603
                break
            k, key = prng.split(key)  # gen:610
            step(cur_len, self._decode_step(cache, t["next_token"], pos))
            pos += 1
        return ModelOutput(sequences=t["sequences"])

    def _sample_group(self, ehs, n_img, N, start_token, max_length, pad_token_id, eos_token_id, prng_key, procs, warp, from_processed: bool):
        """generate(do_sample=True, num_return_sequences=N >= 2): N `_sample` calls over the same images — call n with the key
        `split(PRNGKey(prng_key), N)[n]` — as one decode chain of n_img * N rows, row = image * N + n (cross K/V per image: row_div = N).
        mic_sample_rows_keyed gives row (image, n) the noise of row `image` of call n.  Call n alone would stop once ITS rows have all
        finished (gen:596-603); here its rows ride along until every row has: a finished row only ever receives PAD (gen:629-642) into a
        buffer that is PAD already and leaves its score alone, so that changes nothing (the argument `_run_chain`'s polling relies on).  The
        per-step keys of all draws are walked on the host before the chain starts and copied into the plan's [max_length][N][2] table:
        the step at cur_len reads its N keys from device memory, a captured step holds the table's address, not a call's keys."""
        from . import prng
        from .modeling_clip_vision_mbart import ModelOutput

        dev, st = self.device, self.store
        R = n_img * N
        warp = self._warp_in_force(warp, from_processed)

        def build(plan):
            t = plan.t
            t["sequences"] = torch.empty((R, max_length), dtype=torch.int32, device=dev)
            t["finished"] = torch.empty(R, dtype=torch.int32, device=dev)
            t["next_token"] = torch.empty((R,), dtype=torch.int32, device=dev)
            t["drawn"] = torch.empty((R, 1), dtype=torch.int32, device=dev)
            t["scores"] = torch.empty(R, dtype=torch.float32, device=dev)
            t["keys"] = torch.empty((max_length, N, 2), dtype=torch.int32, device=dev)  # the uint32 key words, bit for bit
            t["pos_all"] = torch.arange(max_length, dtype=torch.int32, device=dev).repeat_interleave(R)
            if warp[0] or warp[1] < 1.0:
                t["thr"] = torch.empty(R, dtype=torch.float32, device=dev)
                t["lim"] = torch.empty(R, dtype=torch.int32, device=dev)

        plan = self._decode_plan(self._plan_key("sample", (n_img, N, max_length, pad_token_id, eos_token_id,
                                                           (procs["min_length"], procs["forced_bos"], procs["forced_eos"]), warp,
                                                           bool(from_processed), self.dtype)), build)
        t = plan.t
        sequences, finished, next_token, scores, keys, pos_all = (t[k] for k in ("sequences", "finished", "next_token", "scores", "keys",
                                                                                 "pos_all"))
        table = prng.step_key_table(prng.split(prng.prng_key(0 if prng_key is None else prng_key), N), max_length)  # gen:561, 610 per draw
        keys.copy_(torch.from_numpy(table.view("int32")))
        sequences.fill_(pad_token_id)
        self._start_tokens(t, sequences[:, 0], next_token, start_token, None, n_img, N)
        finished.zero_()
        scores.zero_()
        cache = self._plan_cache(plan, R, max_length)
        self._decode_set_encoder(cache, ehs.reshape(n_img * st.S, st.d), n_img, N)
        after_decoder = self._sample_step_fn(
            t, R, max_length, pad_token_id, eos_token_id, procs, warp, from_processed,
            lambda cur_len, logits, **kw: ops.sample_rows_keyed(logits, logits.stride(0), st.V, keys[cur_len], t["drawn"], n_img, N,
                                                                finished=finished, score=scores, **kw))

        def step(cur_len):
            with ops.pinned_stream():
                cache["cache_index"] = cur_len - 1
                after_decoder(cur_len, self._decode_step(cache, next_token, pos_all[(cur_len - 1) * R: cur_len * R]))

        _run_chain(plan, step, max_length, lambda: bool(finished.all().item()), _graphs_enabled(dev))
        return ModelOutput(sequences=sequences.clone(), scores=scores.clone())

    # ------------------------------------------------------------------ gen:665-990
    def _decode_slices(self, B: int, K: int) -> int:
        """Number of independent image slices a beam search is cut into (opt-in experiment, default 1 = off).  Images do not interact
        inside a beam-search step, but the reference's STOP test is global over the batch (`beam_search_cond_fn`, gen:798-820:
        `jnp.all(...)` over every image) — one image that can still improve keeps all of them stepping.  Each slice evaluates that
        test over its own images only, so with n > 1 a slice may stop earlier than the reference would have stopped it and its
        sequences / scores can differ from the unsliced search; the default therefore stays at 1.  A decoder step is a chain of ~110
        dependent launches most of which leave the chip idle
        (one 64x64 tile per CU, latency-bound) or use one resource only (decode attention: HBM; GEMMs: MFMA + LDS).  Slices run
        the same chain on their own streams — as parallel branches of the step's hipGraph — so one slice's latency chain and
        HBM-bound kernels overlap another's.  MIC_DECODE_SLICES=n forces n (1 = off)."""
        import os

        want = os.environ.get("MIC_DECODE_SLICES", "auto")
        if self.device.type != "cuda":
            return 1
        n = int(want) if want != "auto" else _AUTO_SLICES
        # auto: a slice keeps at least 256 decoder rows (below that a chain is pure launch latency and slicing only adds launches)
        while n > 1 and (B % n != 0 or (want == "auto" and (B // n) * K < 256)):
            n -= 1
        return max(n, 1)

    def _beam_search(self, ehs, B, K, start_token, max_length, pad_token_id, eos_token_id, length_penalty, early_stopping, procs, lang=None,
                     sl=None, n_best: int = 1):
        """lang = None: one search over B images.  lang = dict(G, start, bos): G searches over the same n_img images in one unsliced
        chain — bookkeeping item i = image * G + g belongs to search g (mic_beam_step_groups), its K rows share the image's cross K/V
        with the rows of the other searches (row_div = G * K).  n_best = N >= 2 (generate(num_return_sequences=N)): the search is the
        same; the result is read at the N best of its K final hypotheses instead of the best alone (host code only)."""
        from .modeling_clip_vision_mbart import ModelOutput

        if 2 * K > 64:
            raise NotImplementedError("num_beams > 32 needs a wider per-row top-k than this build ships (k = 2*num_beams <= 64)")
        dev, st = self.device, self.store
        G = lang["G"] if lang else 1
        n_img, B = B, B * G   # B: bookkeeping items
        NS = 1 if lang else self._decode_slices(B, K)
        Bs = B // NS          # items per slice
        R = Bs * K            # decoder rows per slice

        def build_slice(sub):
            t = sub.t
            t["running_seq"] = torch.empty((Bs, K, max_length), dtype=torch.int32, device=dev)
            t["seq"] = torch.empty((Bs, K, max_length), dtype=torch.int32, device=dev)
            t["finished"] = torch.empty((Bs, K), dtype=torch.int32, device=dev)
            t["running_scores"] = torch.empty((Bs, K), dtype=torch.float32, device=dev)
            t["scores"] = torch.empty((Bs, K), dtype=torch.float32, device=dev)
            t["next_token"] = torch.empty((R,), dtype=torch.int32, device=dev)
            t["src_row"] = torch.empty((R, max_length), dtype=torch.int32, device=dev)
            t["flags"] = torch.empty((Bs, 2), dtype=torch.int32, device=dev)
            t["cand_val"] = torch.empty((R, 2 * K), dtype=torch.float32, device=dev)
            t["cand_idx"] = torch.empty((R, 2 * K), dtype=torch.int32, device=dev)
            t["pos_all"] = torch.arange(max_length, dtype=torch.int32, device=dev).repeat_interleave(R)  # position ids of every step
            t["gstate"] = torch.empty((G, 8) if lang else 8, dtype=torch.int32, device=dev)
            if lang:
                t["start_rows"] = torch.empty(R, dtype=torch.int32, device=dev)
                t["bos_rows"] = torch.empty(R, dtype=torch.int32, device=dev)
            t["score0"] = torch.tensor([0.0] + [NEG] * (K - 1), dtype=torch.float32, device=dev).repeat(Bs, 1).contiguous()
            t["rows"] = torch.arange(R, dtype=torch.int32, device=dev)

        def build(plan):
            plan.subs = [_DecodePlan() for _ in range(NS)]
            for sub in plan.subs:
                build_slice(sub)
            plan.streams = [torch.cuda.Stream(device=dev) for _ in range(NS)] if NS > 1 else []
            plan.shortlist = sl

        plan = self._decode_plan(self._plan_key("beam", (B, K, NS, max_length, pad_token_id, eos_token_id, float(length_penalty),
                                                         bool(early_stopping), procs["min_length"], procs["forced_eos"], self.dtype), lang, sl),
                                 build)
        head = self._shortlist_of(plan, eos_token_id)
        ehs = ehs.reshape(n_img, st.S * st.d)
        steps_fn = []
        for i, sub in enumerate(plan.subs):
            t = sub.t
            t["running_seq"].fill_(pad_token_id)  # gen:751-757
            bos_rows = self._start_tokens(t, t["running_seq"][:, :, 0], t["next_token"], start_token, lang, n_img, K)
            t["seq"].fill_(pad_token_id)
            t["finished"].zero_()  # gen:760
            t["running_scores"].copy_(t["score0"])  # gen:763-765
            t["scores"].fill_(NEG)  # gen:766
            t["src_row"].zero_()
            t["src_row"][:, 0] = t["rows"]
            t["flags"].zero_()
            cache = self._plan_cache(sub, R, max_length)
            cache["src_row"] = t["src_row"]
            cache["ns"] = f"s{i}." if NS > 1 else ""
            # encoder states are shared by an image's K beams (gen:299-307 broadcasts them; here: row r reads image r // K)
            if lang:
                self._decode_set_encoder(cache, ehs.reshape(n_img * st.S, st.d), n_img, G * K)
            else:
                self._decode_set_encoder(cache, ehs[i * Bs:(i + 1) * Bs].reshape(Bs * st.S, st.d), Bs, K)
            t["gstate"].zero_()
            steps_fn.append(self._beam_step_fn(cache, t, Bs, K, max_length, pad_token_id, eos_token_id, length_penalty, early_stopping, procs,
                                               head, groups=G if lang else None, bos_rows=bos_rows))

        def step(cur_len):
            if NS == 1:
                return steps_fn[0](cur_len)
            # fork: every slice's chain on its own stream behind what the current stream has enqueued; join: the current
            # stream waits for all of them (inside a capture these are the graph's parallel branches)
            cur = torch.cuda.current_stream()
            fork = plan.new_event()
            fork.record(cur)
            for i, s_ in enumerate(plan.streams):
                s_.wait_event(fork)
                with torch.cuda.stream(s_):
                    steps_fn[i](cur_len)
                    done = plan.new_event()
                    done.record(s_)
                cur.wait_event(done)

        # the stop flag and step count of every search: word 3 and 4 of a slice's gstate [8], of row g of a grouped call's [G, 8] (a
        # search that has stopped leaves its state alone while its rows ride along: its outputs are those of the separate call that
        # stopped there).  The chain ends when every search of every slice has stopped: one host read per slice and poll.
        gstates = [sub.t["gstate"].view(-1, 8) for sub in plan.subs]
        _run_chain(plan, step, max_length, lambda: all(bool((g[:, 3] != 0).all().item()) for g in gstates), _graphs_enabled(dev, NS))
        out = ModelOutput(**self._beam_result([sub.t for sub in plan.subs], n_best, G if lang else None))
        steps = [g[:, 4].tolist() for g in gstates]
        out["steps"] = steps[0] if lang else max(s[0] for s in steps)
        return out

    @classmethod
    def _beam_result(cls, slices, n_best: int, groups=None) -> dict:
        """gen:980-990 over the state tensors of every slice: an item with a finished hypothesis returns its finished ones, any other
        its running ones; the n_best best of them, slices concatenated — sequences [items * n_best, max_length], scores
        [items * n_best], row item * n_best + j.  groups = G (a grouped call, item = image * G + g): [G, images * n_best, max_length]
        and [G, images * n_best]."""
        outs = []
        for t in slices:
            any_fin = t["finished"].bool().any(dim=1)  # gen:980
            outs.append(cls._n_best(torch.where(any_fin[:, None, None], t["seq"], t["running_seq"]),  # gen:981-983
                                    torch.where(any_fin[:, None], t["scores"], t["running_scores"]), n_best))  # gen:984
        seq, scores = torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        L = seq.shape[-1]
        if groups is None:
            return dict(sequences=seq.reshape(-1, L).contiguous(), scores=scores.reshape(-1).contiguous())
        images = seq.shape[0] // groups
        return dict(sequences=seq.view(images, groups, n_best, L).transpose(0, 1).reshape(groups, images * n_best, L).contiguous(),
                    scores=scores.view(images, groups, n_best).transpose(0, 1).reshape(groups, images * n_best).contiguous())

    @staticmethod
    def _n_best(out_seq, out_scores, n_best: int):
        """gen:987-990 at columns K-1, K-2, ..., K-n_best instead of -1 alone: the state is sorted ascending (best last), so the n_best
        best hypotheses of every item, best first — [items, n_best, max_length] and [items, n_best].  Slots that never held a finished
        hypothesis come back as they lie in the state (PAD rows, score NEG)."""
        return out_seq.flip(1)[:, :n_best].contiguous(), out_scores.flip(1)[:, :n_best].contiguous()

    def _beam_step_fn(self, cache, t, B, K, max_length, pad_token_id, eos_token_id, length_penalty, early_stopping, procs, head, groups=None,
                      bos_rows=None):
        """the launches of one beam-search step (gen:822-966) of one slice of B items: step(cur_len).  head: `_shortlist_of`'s tuple (with
        a vocabulary shortlist the head and the top-k run over its columns, the candidates leave as vocabulary ids: mic_beam_step sees
        no difference); groups = G: the items belong to G searches (item i to search i % G, gstate [G][8]); bos_rows: per-row
        ForcedBOS ids of such a call"""
        st = self.store
        R = B * K
        running_seq, seq, finished, running_scores, scores = t["running_seq"], t["seq"], t["finished"], t["running_scores"], t["scores"]
        next_token, src_row, flags, cand_val, cand_idx, pos_all, gstate = (t[k] for k in ("next_token", "src_row", "flags", "cand_val",
                                                                                          "cand_idx", "pos_all", "gstate"))

        def step(cur_len):
            with ops.pinned_stream():
                cache["cache_index"] = cur_len - 1
                logits, stat = self._decode_step(cache, next_token, pos_all[(cur_len - 1) * R: cur_len * R], stats=True, shortlist=head[0])  # gen:830-840
                self._candidates(logits, stat, head, 2 * K, R, cand_val, cand_idx, procs, cur_len, max_length, bos_rows,
                                 row_bias=running_scores.reshape(-1))  # gen:850-873
                ops.beam_step(B, K, max_length, st.V, cur_len, eos_token_id, pad_token_id, length_penalty, early_stopping, cand_val,
                              cand_idx, running_seq, running_scores, seq, scores, finished, src_row, next_token, flags, gstate=gstate,
                              groups=groups)  # gen:872-966
        return step
