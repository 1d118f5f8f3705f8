"""Data-parallel training step with the reference's semantics (`main.py:281-292, 629-635, 658-707, 710-721`):

    loss, grads = value_and_grad(compute_loss)(params)      # per-rank masked-mean loss on the local shard (main.py:679)
    grads = pmean(grads)                                     # RCCL all-reduce over xGMI, bucketed, overlapped (main.py:698)
    params = adamw(params, grads)                            # identical local update on every rank (main.py:701)
    metrics = pmean({loss, learning_rate})                   # main.py:703-704

One process per GPU (`torch.distributed`, backend "nccl" = RCCL on ROCm; "gloo" on CPU for the tests of the host logic).
Gradients live in ONE flat fp32 buffer ordered as backward completes them, so buckets are contiguous slices; each
bucket's all-reduce is issued on a side HIP stream as soon as backward has produced it (event-ordered), overlapping the
rest of backward; AdamW waits on the side stream once.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops


def shift_tokens_right(input_ids: np.ndarray, pad_token_id: int) -> np.ndarray:
    """main.py:362-369."""
    shifted = np.zeros(input_ids.shape, dtype=np.int64)
    shifted[:, 1:] = input_ids[:, :-1]
    shifted[:, 0] = pad_token_id
    return shifted


def create_learning_rate_fn(train_ds_size: int, train_batch_size: int, num_train_epochs: int, num_warmup_steps: int,
                            learning_rate: float) -> Callable[[int], float]:
    """main.py:281-292: linear warmup 0->lr over `num_warmup_steps`, then linear decay lr->0 over the remaining steps."""
    steps_per_epoch = train_ds_size // train_batch_size
    num_train_steps = steps_per_epoch * num_train_epochs

    def schedule(step: int) -> float:
        if step < num_warmup_steps:
            frac = min(max(step / num_warmup_steps, 0.0), 1.0) if num_warmup_steps > 0 else 1.0
            return learning_rate * frac
        n = num_train_steps - num_warmup_steps
        if n <= 0:  # optax.linear_schedule with transition_steps <= 0 is the constant init_value
            return learning_rate
        frac = min(max((step - num_warmup_steps) / n, 0.0), 1.0)
        return learning_rate + (0.0 - learning_rate) * frac

    return schedule


def loss_rows(attention_mask, labels):
    """Collate-side helper: flat indices of the label positions whose loss mask is 1 (row-major over [B,T]) and the labels
    at those positions.  `Trainer` runs the LM head / cross-entropy only there (exact: main.py:678 multiplies the rest by 0).
    Returns (idx int32 [Mc], labels int32 [Mc]) as numpy arrays."""
    m = np.asarray(attention_mask).reshape(-1)
    idx = np.nonzero(m)[0].astype(np.int32)
    return idx, np.asarray(labels).reshape(-1)[idx].astype(np.int32)


def packed_rows(attention_mask, decoder_input_ids):
    """Collate-side helper for the packed decoder: when every row of the [B,T] loss / attention mask is a PREFIX of ones (what
    the tokenizer's `padding="max_length"` produces, main.py:513-523), the decoder can run on the sum(len_b) valid positions
    only — sequence b = packed rows [q_off[b], q_off[b] + q_len[b]), in the same order as `loss_rows`' indices.  Returns
    (q_off int32 [B], q_len int32 [B], ids int32 [B*T], pos int32 [B*T]) — decoder input ids and position ids of the packed
    rows, zero-padded to B*T — or None when some row is not a prefix (the padded path is used then)."""
    m = np.asarray(attention_mask)
    B, T = m.shape
    ln = m.astype(bool).sum(1).astype(np.int32)
    if not np.array_equal(m.astype(bool), np.arange(T)[None, :] < ln[:, None]):
        return None
    off = np.zeros(B, dtype=np.int32)
    off[1:] = np.cumsum(ln)[:-1]
    idx = np.nonzero(m.reshape(-1))[0]
    ids = np.zeros(B * T, dtype=np.int32)
    pos = np.zeros(B * T, dtype=np.int32)
    ids[: idx.size] = np.asarray(decoder_input_ids).reshape(-1)[idx]
    pos[: idx.size] = (idx % T).astype(np.int32)  # default position ids arange(T) (modeling:490-494)
    return off, ln, ids, pos


def group_packed_rows(q_off, q_len, captions_per_image: int):
    """Packed rows of G = captions_per_image captions per image, image-major (caption b belongs to image b // G): an image's G
    captions are consecutive packed rows, so for the cross-attention — which couples no two queries — image i is ONE sequence of
    q_len'[i] = sum_g q_len[i*G + g] rows starting at q_off'[i] = q_off[i*G].  Returns (q_off', q_len') int32 [B // G]; G = 1 is the
    identity.  Pure host function (numpy)."""
    off, ln = np.asarray(q_off, dtype=np.int32), np.asarray(q_len, dtype=np.int32)
    G = int(captions_per_image)
    if G < 1 or off.shape != ln.shape or off.ndim != 1 or off.size % G:
        raise ValueError(f"group_packed_rows: {off.size} sequences do not divide into groups of {captions_per_image}")
    if off.size and not np.array_equal(off[1:], (off + ln)[:-1]):
        raise ValueError("group_packed_rows: the packed sequences must follow one another without gaps (packed_rows' layout)")
    return off[::G].copy(), ln.reshape(-1, G).sum(1).astype(np.int32)


def check_captions_per_image(batch, fp8: bool = False) -> int:
    """batch["captions_per_image"] = G (absent: 1), checked on the host before anything touches a device: an int >= 1, caption
    rows == images * G, and no fp8 GEMMs with G > 1.  Returns G."""
    G = batch.get("captions_per_image", 1)
    if isinstance(G, (bool, np.bool_)) or not isinstance(G, (int, np.integer)) or G < 1:
        raise ValueError(f"batch['captions_per_image'] must be an integer >= 1, got {G!r}")
    G = int(G)
    n_img, n_cap = int(batch["pixel_values"].shape[0]), int(batch["input_ids"].shape[0])
    if n_cap != n_img * G:
        raise ValueError(f"batch['captions_per_image'] = {G}: {n_img} images need {n_img * G} caption rows (image-major: row r belongs to "
                         f"image r // {G}), got {n_cap}")
    if G > 1 and fp8:
        raise ValueError("captions_per_image > 1 is not supported together with gemm_dtype='fp8' (out of scope: the fused e5m2 emission "
                         "of the cross-attention's dK / dV has no shared form)")
    return G


def check_loss_weights(batch, fp8: bool = False):
    """batch["loss_weights"] (absent: None), checked on the host before anything touches a device: float weights of shape [R] (one
    per caption row) or [R, T] (one per token), R, T = batch["input_ids"].shape; no fp8 GEMMs.  A host array must be finite and is
    returned as a float32 numpy array; a device tensor is returned as it is — its shape is checked, its values are trusted (looking
    at them would put a device-to-host sync into every step, like `packed_rows`)."""
    w = batch.get("loss_weights")
    if w is None:
        return None
    if fp8:
        raise ValueError("batch['loss_weights'] is not supported together with gemm_dtype='fp8' (out of scope: the e5m2 dlogits of the "
                         "fp8 LM head carry a closed-form scale that rests on |g| <= 1)")
    R, T = (int(x) for x in batch["input_ids"].shape)
    on_device = isinstance(w, torch.Tensor) and w.device.type != "cpu"
    if not on_device:
        w = w.numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
        if w.dtype == object or not (np.issubdtype(w.dtype, np.floating) or np.issubdtype(w.dtype, np.integer)):
            raise ValueError(f"batch['loss_weights'] must hold real numbers, got dtype {w.dtype}")
    elif not (w.is_floating_point() or w.dtype in (torch.int32, torch.int64)):
        raise ValueError(f"batch['loss_weights'] must hold real numbers, got dtype {w.dtype}")
    if tuple(w.shape) not in ((R,), (R, T)):
        raise ValueError(f"batch['loss_weights'] must have shape [{R}] (one weight per caption row) or [{R}, {T}] (one per token), got "
                         f"{list(w.shape)}")
    if on_device:
        return w
    w = w.astype(np.float32)
    if not np.isfinite(w).all():
        raise ValueError("batch['loss_weights'] holds non-finite values (NaN or inf)")
    return w


def plan_buckets(numel: int, bucket_elems: int, boundaries: List[int], max_elems: int = 0,
                 splittable: Tuple[Tuple[int, int, int], ...] = ()) -> List[Tuple[int, int]]:
    """Contiguous [begin, end) slices of the flat gradient buffer, cut at segment boundaries, each >= bucket_elems
    (except the last).  `max_elems` > 0: a slice larger than that is cut further, but only INSIDE the segments listed in
    `splittable` ((begin, end, align): cuts at begin + k * step, step = the largest multiple of `align` <= max_elems) — the tied
    embedding is ONE segment of 256 M elements (1 GB in fp32): whole, its optimizer pass could not start before the last byte of
    its all-reduce had arrived.  Pure host logic (tested on CPU)."""
    cuts, start = [], 0
    for b in sorted(set(boundaries)):
        if b - start >= bucket_elems and b < numel:
            cuts.append((start, b))
            start = b
    cuts.append((start, numel))
    if max_elems <= 0:
        return cuts
    out = []
    for (b, e) in cuts:
        pts = set()
        if e - b > max_elems:
            for (sb, se, align) in splittable:
                step = max(align, (max_elems // align) * align)
                x = sb + step
                while x < min(e, se):
                    if x > b:
                        pts.add(x)
                    x += step
        edges = [b] + sorted(pts) + [e]
        out += [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]
    return out


MAX_BUCKET_MB = 128.0  # largest piece of the tied embedding that goes on the wire as one collective


TAIL_BUCKET_MB = 12.0  # the LAST bucket (what backward completes last = what the next forward reads first) is kept this small


def bucket_plan(store, bucket_mb: float = 64.0, max_mb: float = MAX_BUCKET_MB, tail_mb: float = TAIL_BUCKET_MB) -> List[Tuple[int, int]]:
    """the gradient-exchange buckets of a ParamStore layout (a store built with allocate=False is enough): >= bucket_mb each, cut
    at segment boundaries in the order backward completes them; the tied embedding in pieces of <= max_mb (whole rows).
    tail_mb > 0: the last bucket is cut once more, at the latest segment boundary that leaves a final piece of at most tail_mb —
    its exchange and optimizer pass are the serial tail of the step (nothing is left to hide them under, and the next forward pass
    starts with exactly these weights): 12 MB of patch embedding / position / pre-LayerNorm parameters instead of 64+ MB."""
    bounds = [s.offset for s in store.segs.values()]
    sh = store.segs["shared"]
    split = ((sh.offset, sh.offset + sh.numel, store.d),) if sh.numel % store.d == 0 else ()
    out = plan_buckets(store.numel, int(bucket_mb * 1024 * 1024 / 4), bounds, max_elems=int(max(max_mb, bucket_mb) * 1024 * 1024 / 4),
                       splittable=split)
    if tail_mb > 0:
        # (the very last bucket is the small region of atomically accumulated bias / LayerNorm gradients; the one in front of it ends
        # with the patch embedding) ... and the piece in front of those to ~3 x that (one ViT layer): its pass is released by the
        # last layer's backward and has the patch-embedding kernels left to hide under
        for k, lim_mb in ((1, tail_mb), (2, tail_mb), (3, 3.0 * tail_mb)):
            if len(out) < k:
                break
            b, e = out[-k]
            lim = int(lim_mb * 1024 * 1024 / 4)
            inside = sorted(x for x in set(bounds) if b < x < e and e - x <= lim)
            if e - b > lim and inside:
                out[len(out) - k:len(out) - k + 1] = [(b, inside[0]), (inside[0], e)]
    return out


def describe_buckets(store, buckets: List[Tuple[int, int]], comm_bytes: int = 4) -> List[Dict]:
    """per bucket: first / last segment it covers, elements and bytes on the wire per rank and exchange (logged by rank 0 at
    Trainer construction; the order is the order backward completes them)"""
    segs = sorted(store.segs.values(), key=lambda s: s.offset)
    out = []
    for i, (b, e) in enumerate(buckets):
        inside = [s.name for s in segs if s.offset < e and s.offset + s.numel > b]
        out.append({"bucket": i, "begin": b, "end": e, "elements": e - b, "MB": round((e - b) * comm_bytes / 1e6, 1),
                    "first": inside[0], "last": inside[-1], "segments": len(inside)})
    return out


# ---- what the gradient exchange costs, from byte counts (no N > 1 hardware has been available to measure it)
XGMI_LINK_GBPS = 64.0      # per direction and peer link, what a ring gets out of one xGMI link (7 links x ~153 GB/s bidirectional per GPU)
BACKWARD_WINDOW_MS = 13.0  # backward of the batch-64 step: the time the exchange can hide under (profiles/README.md)
COMM_CUS_DEFAULT = 32      # RCCL channels (= persistent blocks, one CU each) `configure_rccl` caps the collectives at


def configure_rccl(max_channels: int = COMM_CUS_DEFAULT) -> int:
    """Call BEFORE `torch.distributed.init_process_group("nccl")`: caps the CUs RCCL's collectives can occupy by bounding its channel
    count (one persistent block per channel, one CU each): `NCCL_MAX_NCHANNELS` (and `NCCL_MIN_NCHANNELS` no larger than that).  A
    value the user already exported wins.  Returns the cap now in force; `Trainer` reads it back (`rccl_channel_cap`) as its
    `comm_cus` default, so the CU budget the GEMM tile planner works with is the number RCCL was actually held to — not an assumption."""
    import os

    cap = int(os.environ.setdefault("NCCL_MAX_NCHANNELS", str(int(max_channels))))
    lo = os.environ.get("NCCL_MIN_NCHANNELS")
    if lo is not None and int(lo) > cap:
        os.environ["NCCL_MIN_NCHANNELS"] = str(cap)
    return cap


def rccl_channel_cap() -> int:
    """the channel cap exported to RCCL (`configure_rccl` or the user's environment); 0 = none: RCCL picks its own count"""
    import os

    try:
        return max(0, int(os.environ.get("NCCL_MAX_NCHANNELS", "0")))
    except ValueError:
        return 0


XGMI_LINK_PEAK_GBPS = 153.0  # per peer link as the hardware guide and SURVEY §5 quote it (the optimistic end of the projection)


def allreduce_ms(nbytes: float, world: int, link_gbps: float = XGMI_LINK_GBPS, algo: str = "all_links") -> float:
    """PROJECTED all-reduce time of `nbytes` per rank among `world` fully connected GPUs (no N > 1 hardware run has been possible:
    a byte-count model, not a measurement).
    algo="all_links" (default): every rank sends and receives 2 (world-1)/world of its bytes spread over its world-1 peer links —
      what a direct reduce-scatter + all-gather does, and what world-1 concurrent rings do: 2 nbytes / (world * link).
    algo="ring_one_link": a single classic ring, one link per direction: 2 (world-1)/world * nbytes / link.
    `link_gbps`: XGMI_LINK_GBPS (64, the conservative default: what RCCL rings have been seen to get out of one link) or
    XGMI_LINK_PEAK_GBPS (153, SURVEY §5's direct RS + AG figure: 3.6 ms for the 2.19 GB fp32 gradient at N = 8)."""
    if world <= 1:
        return 0.0
    if algo == "ring_one_link":
        return 2.0 * (world - 1) / world * nbytes / (link_gbps * 1e9) * 1e3
    if algo != "all_links":
        raise ValueError(f"unknown all-reduce model {algo!r}")
    return 2.0 * nbytes / (world * link_gbps * 1e9) * 1e3


def allreduce_projections(nbytes: float, world: int) -> Dict[str, float]:
    """the bracket the byte-count model gives: pessimistic (all links at 64 GB/s — what `choose_comm_dtype` and the emulated
    exchange use), optimistic (direct reduce-scatter + all-gather over all links at 153 GB/s) and a single ring"""
    return {"all_links_64GBps_ms": round(allreduce_ms(nbytes, world), 2),
            "direct_rs_ag_153GBps_ms": round(allreduce_ms(nbytes, world, XGMI_LINK_PEAK_GBPS), 2),
            "single_ring_153GBps_ms": round(allreduce_ms(nbytes, world, XGMI_LINK_PEAK_GBPS, "ring_one_link"), 2)}


def choose_comm_dtype(world: int, numel: int, window_ms: float = BACKWARD_WINDOW_MS, link_gbps: float = XGMI_LINK_GBPS) -> Optional[torch.dtype]:
    """`grad_comm_dtype="auto"`: fp32 — the reference's `lax.pmean` of fp32 gradients (main.py:698) — wherever the projected fp32
    exchange fits under backward, bf16 where it would not (the step would be communication-bound; a bf16 sum changes pmean's
    arithmetic by one rounding per rank and element, tests/test_ddp_gpu.py).  By the byte counts of the 547 M-parameter model at
    the conservative 64 GB/s per link: N = 2: 34 ms, N = 4: 17 ms -> bf16 (17 / 8.5 ms); N = 8: 8.5 ms -> fp32.  With
    `link_gbps=XGMI_LINK_PEAK_GBPS` (direct reduce-scatter + all-gather at 153 GB/s: 14.3 / 7.2 / 3.6 ms) only N = 2 is over the
    window; pass the link rate RCCL was MEASURED at once a multi-GPU node has run tools/first_multi_gpu_run.sh."""
    if world <= 1 or allreduce_ms(4.0 * numel, world, link_gbps) <= window_ms:
        return None
    return torch.bfloat16


class GradReducer:
    """Bucketed all-reduce(mean) of the flat gradient buffer on a side stream (C1 of SURVEY §2.3), followed — on a third stream —
    by a per-bucket callback (the fused AdamW of that slice): HBM-bound optimizer traffic then overlaps the MFMA-bound remainder
    of backward instead of trailing it.

    ONE ordering rule per bucket, `ready_when[i]`: when may the bucket's optimizer pass be issued, beyond "its exchange is done"?
      "exchanged"  right behind the exchange (the default);
      "next"       at the next progress report, behind everything backward has enqueued by then — a kernel issued right after
                   the gradient became final still READS the weights (the LM head's dX GEMM reads the tied embedding);
      "end"        in finish(), after `before()` — the gradient receives a late part (the sparse input-embedding rows).

    Per step (`start_step`), for gradient accumulation: `local=True` issues no exchange at all (a micro-step whose gradient only joins
    the running sum), `on_ready` / `ready_when` replace the callback and its ordering rule for that step, and `pre_exchange(b, e)` runs
    on the collective stream in front of the bucket's all-reduce (the running sum joins the gradient there).
    """

    def __init__(self, flat_grad: torch.Tensor, buckets: List[Tuple[int, int]], group=None, on_ready=None,
                 ready_when: Optional[List[str]] = None, comm_dtype: Optional[torch.dtype] = None, opt_cus: int = 0,
                 emulate: Optional[Dict] = None):
        """opt_cus: CUs of the optimizer stream's mask (0: no mask).  emulate (one GPU only, bench.py --emulate-comm):
        {"world": N, "cus": CUs of the collective stream, "comm_bytes": bytes per element on the wire} — every bucket's exchange
        is replaced by a kernel that occupies `cus` CUs for the projected duration of that bucket's all-reduce."""
        import torch.distributed as dist

        self.dist, self.group = dist, group
        self.grad, self.buckets = flat_grad, buckets
        self.ready_when = list(ready_when) if ready_when is not None else ["exchanged"] * len(buckets)
        assert len(self.ready_when) == len(buckets) and all(w in ("exchanged", "next", "end") for w in self.ready_when)
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.cuda = flat_grad.is_cuda
        self.stream = ops.role_stream(flat_grad.device, "collective") if self.cuda else None    # collectives
        self.opt_stream = ops.role_stream(flat_grad.device, "optimizer") if self.cuda else None  # per-bucket optimizer work
        # ... on CUs of its own (`opt_cus` of them; 0 = no mask): the optimizer is HBM-bound and needs few CUs, while the backward
        # GEMM blocks own a CU's whole register file and never share one — with a mask the two run side by side instead of taking
        # turns.  A CU-masked HIP stream is a BLOCKING stream (it synchronises with the null stream, torch's default): the step then
        # runs on `step_stream`, and the passes postponed to the end of backward on the unmasked `tail_stream`.
        self.step_stream = self.tail_stream = None
        self.emulate = dict(emulate) if (emulate and self.cuda and self.world == 1) else None
        if self.cuda and on_ready is not None and opt_cus > 0:
            try:
                self.opt_stream = ops.cu_masked_stream(0, opt_cus, flat_grad.device)
                self.step_stream = ops.role_stream(flat_grad.device, "step")
                self.tail_stream = ops.role_stream(flat_grad.device, "tail")
            except Exception as ex:  # the stack refuses CU masks: plain streams, as before
                import sys

                print(f"[mic_amd.GradReducer] no CU-masked optimizer stream ({ex}); using a plain stream", file=sys.stderr)
        if self.emulate is not None:
            # the stand-in collectives sit on the LAST `cus` bits of the CU mask (the optimizer's mask starts at bit 0)
            cus = int(self.emulate.get("cus", COMM_CUS_DEFAULT))
            self.stream = ops.cu_masked_stream(256 - cus, cus, flat_grad.device)
            if self.step_stream is None:  # a masked stream is a blocking stream: keep the step off the null stream
                self.step_stream = ops.role_stream(flat_grad.device, "step")
            self._emu_scratch = torch.empty(max(e - b for b, e in buckets), dtype=flat_grad.dtype, device=flat_grad.device)
            self.emulated_ms = 0.0
            self.emulated_events = []
        self.on_ready = on_ready if self.cuda else None
        self._cb, self._when, self._local, self._pre = self.on_ready, self.ready_when, False, None  # this step's (start_step)
        self._finishing = False
        self.host_s = 0.0
        self.next = 0
        self.handles = []
        self._pending: List[Tuple[int, int, object]] = []  # "next": exchange started, optimizer pass due at the next report
        self._at_end: List[Tuple[int, int]] = []           # "end"
        # opt-in reduced-precision exchange (e.g. torch.bfloat16): every rank rounds its bucket, the collective sums in that
        # dtype, the result is widened back into the fp32 buffer.  Halves the xGMI bytes; NOT the reference's fp32 pmean.
        self.comm_dtype = comm_dtype if (comm_dtype is not None and comm_dtype != flat_grad.dtype) else None
        # two staging buffers used alternately: the narrowing copy of bucket k+1 does not wait for the widening copy of bucket k
        self.stage = ([torch.empty(max(e - b for b, e in buckets), dtype=self.comm_dtype, device=flat_grad.device) for _ in range(2)]
                      if self.comm_dtype is not None and self.world > 1 else None)
        self._stage_i = 0

    def _all_reduce(self, b: int, e: int, async_op: bool = False):
        if self.stage is None:
            return self.dist.all_reduce(self.grad[b:e], op=self.dist.ReduceOp.SUM, group=self.group, async_op=async_op)
        st = self.stage[self._stage_i][: e - b]
        self._stage_i ^= 1
        st.copy_(self.grad[b:e])
        self.dist.all_reduce(st, op=self.dist.ReduceOp.SUM, group=self.group)
        self.grad[b:e].copy_(st)
        return None

    def _emulated_exchange(self, b: int, e: int):
        """one GPU: hold the collective stream's CUs for as long as the all-reduce of this bucket is projected to take"""
        em = self.emulate
        nbytes = (e - b) * int(em.get("comm_bytes", 4))
        ms = allreduce_ms(nbytes, int(em["world"]), float(em.get("link_gbps", XGMI_LINK_GBPS)))
        self.emulated_ms += ms
        ev = None
        if em.get("timing"):  # bench.py: how long the stand-in kernels really held the stream
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        with ops.pinned_stream():
            ops.comm_emulate(self.grad[b:e], self._emu_scratch[: e - b], (e - b) * self.grad.element_size(), ms * 1e3,
                             2 * int(em.get("cus", COMM_CUS_DEFAULT)))
        if ev is not None:
            ev[1].record()
            self.emulated_events.append(ev)

    @property
    def active(self) -> bool:
        return self.world > 1 or self._cb is not None or self.emulate is not None  # (_cb: this step's callback, see start_step)

    def start_step(self, local: bool = False, on_ready=None, ready_when: Optional[List[str]] = None, pre_exchange=None):
        """local: no exchange this step, whatever the world size.  on_ready / ready_when: this step's per-bucket callback and its
        ordering rules (default: the constructor's).  pre_exchange(b, e): on the collective stream, in front of the bucket's all-reduce."""
        self._local, self._pre = bool(local), pre_exchange
        self._cb = on_ready if (on_ready is not None and self.cuda) else self.on_ready
        self._when = list(ready_when) if ready_when is not None else self.ready_when
        assert len(self._when) == len(self.buckets)
        self.host_s = 0.0
        self.next = 0
        self.handles = []
        self._pending = []
        self._at_end = []
        if self.emulate is not None:
            self.emulated_ms = 0.0
            self.emulated_events = []

    def _issue(self, b: int, e: int, ev, here=None):
        """the bucket's optimizer pass on the optimizer stream, behind its exchange (`ev`) and, for "next" buckets, behind
        everything the step's stream had enqueued at the report that released them (`here`).  Buckets released by finish() — backward
        is over, nothing shares the chip with them — go to the UNMASKED tail stream when the optimizer stream is restricted to a few
        CUs: the pass is HBM-bound and the step waits for it."""
        st = self.tail_stream if (self._finishing and self.tail_stream is not None) else self.opt_stream
        with torch.cuda.stream(st):
            st.wait_event(ev)
            if here is not None:
                st.wait_event(here)
            with ops.pinned_stream():  # launch on that stream, not on the step's pinned main stream
                self._cb(b, e)

    def _issue_pending(self):
        if not self._pending:
            return
        here = torch.cuda.Event()
        here.record(torch.cuda.current_stream())
        for (b, e, ev) in self._pending:
            self._issue(b, e, ev, here)
        self._pending = []

    def progress(self, offset_done: int):
        """Backward reports that every gradient with flat offset < offset_done is final."""
        if not self.active:
            return
        import time

        t0 = time.perf_counter()
        try:
            self._progress(offset_done)
        finally:
            self.host_s += time.perf_counter() - t0  # host time this step spent issuing exchanges / optimizer passes (bench.py reports it)

    def _progress(self, offset_done: int):
        if self.cuda:
            self._issue_pending()
        while self.next < len(self.buckets) and self.buckets[self.next][1] <= offset_done:
            b, e = self.buckets[self.next]
            when = self._when[self.next]
            if self.cuda:
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream())
                if (self.world > 1 or self.emulate is not None) and not self._local:
                    with torch.cuda.stream(self.stream):
                        self.stream.wait_event(ev)
                        if self._pre is not None:
                            with ops.pinned_stream():
                                self._pre(b, e)
                        if self.world > 1:
                            self._all_reduce(b, e)
                        else:
                            self._emulated_exchange(b, e)
                        ev = torch.cuda.Event()
                        ev.record(self.stream)
                if self._cb is None:
                    pass
                elif when == "end":
                    self._at_end.append((b, e))
                elif when == "next":
                    self._pending.append((b, e, ev))
                else:
                    self._issue(b, e, ev)
            elif not self._local:  # CPU tensors (host-logic tests over gloo)
                if self._pre is not None:
                    self._pre(b, e)
                h = self._all_reduce(b, e, async_op=True)
                if h is not None:
                    self.handles.append(h)
            self.next += 1

    def finish(self, before=None, after=None):
        """End of backward: the remaining buckets go out; then, behind every collective and everything backward has enqueued,
        `before()` (the sparse embedding-row exchange), the optimizer passes of the "end" buckets and `after()` (the part of the
        optimizer that needed `before`); finally the step's stream waits for the side streams."""
        self._finishing = True
        try:
            self.progress(self.grad.numel())
        finally:
            self._finishing = False
        if not self.active:
            return
        import time

        t0 = time.perf_counter()
        try:
            self._finish(before, after)
        finally:
            self.host_s += time.perf_counter() - t0

    def _finish(self, before, after):
        if not self.cuda:
            for h in self.handles:
                h.wait()
            return
        self._issue_pending()
        if self._cb is None:
            after = None  # the late pass belongs to the per-bucket optimizer
            self._at_end = []
        cur = torch.cuda.current_stream()
        if self._at_end or before is not None or after is not None:
            # these run after backward, with nothing beside them: on the unmasked tail stream when the optimizer stream is
            # restricted to a few CUs
            tail = self.tail_stream if self.tail_stream is not None else self.opt_stream
            with torch.cuda.stream(tail):
                if self.world > 1 or self.emulate is not None:
                    tail.wait_stream(self.stream)
                if tail is not self.opt_stream:
                    tail.wait_stream(self.opt_stream)
                tail.wait_stream(cur)  # the end of backward (the sparse embedding rows come from there)
                with ops.pinned_stream():
                    if before is not None:
                        before()
                    for (b, e) in self._at_end:
                        self._cb(b, e)
                    if after is not None:
                        after()
            if tail is not self.opt_stream:
                self.opt_stream.wait_stream(tail)
            self._at_end = []
        cur.wait_stream(self.stream)
        cur.wait_stream(self.opt_stream)
        if self.tail_stream is not None and self.tail_stream is not self.opt_stream:
            # the optimizer passes of the buckets finish() released ran on the tail stream (`_issue`): without this join the next forward
            # pass could read weights those passes were still writing whenever nothing else had been queued there (found by making a side
            # stream lag: tests/test_fp8_gpu.py::test_fp8_weight_copies_made_on_a_lagging_side_stream_are_waited_for)
            cur.wait_stream(self.tail_stream)


OPT_CUS_DEFAULT = 96  # CUs of the optimizer stream (12 per XCD of an MI355X): profiles/README.md, round 3 A/B


def virtual_rank_dropout_seed(seed: int, rank: int, step: int, accumulate_steps: int = 1, micro_step: int = 0) -> int:
    """Dropout seed of one forward/backward pass.  Micro-step j of rank r under `accumulate_steps=N` draws the stream of VIRTUAL rank
    r * N + j: the per-device stream (main.py:251) of that rank, split per optimizer step (main.py:686) — so N micro-steps on one
    GPU draw the masks N ranks would draw, and W ranks x N micro-steps those of W * N ranks.  N = 1, j = 0: what `Trainer` uses
    without accumulation.  Pure host arithmetic."""
    vrank = int(rank) * int(accumulate_steps) + int(micro_step)
    stream = (int(seed) * 1000003 + vrank * 7919) & 0xFFFFFFFF
    return (stream + int(step) * 0x9E3779B1) & 0xFFFFFFFF


# ---- parameter groups (Trainer(param_groups=...)): ready-made matchers over the ParamStore segment names, applied with re.fullmatch
ENCODER = r"vit.*|patch\.w"   # the image tower: every vit* segment and the patch embedding; the bridge vp.* is not part of it
NO_DECAY = r".*\.[bg]|flb"    # biases and LayerNorm scales / biases (HF's decay mask); the embeddings (shared, dec.pos, vit.pos, vit.cls) decay
_GROUP_KEYS = ("match", "lr_scale", "weight_decay", "frozen")


def _check_param_groups(param_groups) -> None:
    """the part of the validation that needs no store: shape of the argument, keys, value ranges (ValueError)"""
    import math
    import numbers

    if not isinstance(param_groups, list) or not all(isinstance(g, dict) for g in param_groups):
        raise ValueError(f"param_groups must be None or a list of dicts, got {type(param_groups).__name__}")
    for i, g in enumerate(param_groups):
        unknown = sorted(set(g) - set(_GROUP_KEYS), key=str)
        if unknown:
            raise ValueError(f"param_groups[{i}]: unknown key(s) {unknown}; known: {list(_GROUP_KEYS)}")
        if "match" not in g:
            raise ValueError(f"param_groups[{i}]: 'match' is missing")
        mt = g["match"]
        if not (isinstance(mt, str) or callable(mt) or (isinstance(mt, (list, tuple)) and mt and all(isinstance(x, str) for x in mt))):
            raise ValueError(f"param_groups[{i}]: 'match' must be a regex string, a non-empty list of regex strings or a callable, got {mt!r}")
        for key, low in (("lr_scale", 0.0), ("weight_decay", None)):
            if key in g:
                x = g[key]
                if (isinstance(x, (bool, np.bool_)) or not isinstance(x, numbers.Real) or not math.isfinite(x)
                        or (low is not None and x < low)):
                    raise ValueError(f"param_groups[{i}]: {key} must be a finite real number{' >= 0' if low is not None else ''}, got {x!r}")
        if "frozen" in g and not isinstance(g["frozen"], (bool, np.bool_)):
            raise ValueError(f"param_groups[{i}]: frozen must be a bool, got {g['frozen']!r}")


def _segment_groups(store, param_groups, weight_decay: float) -> List[Tuple[str, int, float, float, bool]]:
    """[(segment, offset, lr_scale, wd, frozen)] in flat order: the first matching group wins, an unmatched segment keeps
    (1, weight_decay, False).  ValueError for a malformed argument and for a group that matches no segment."""
    import re

    _check_param_groups(param_groups)

    def matcher(mt):
        if callable(mt):
            return lambda name: bool(mt(name))
        pats = [re.compile(x) for x in ([mt] if isinstance(mt, str) else mt)]
        return lambda name: any(p.fullmatch(name) for p in pats)

    fns = [matcher(g["match"]) for g in param_groups]
    hits = [0] * len(fns)
    out = []
    for s in sorted(store.segs.values(), key=lambda s: s.offset):
        lr_scale, wd, frozen = 1.0, float(weight_decay), False
        first = True
        for i, (fn, g) in enumerate(zip(fns, param_groups)):
            if fn(s.name):
                hits[i] += 1  # (a group shadowed everywhere by earlier ones still names real segments: not an error)
                if first:
                    lr_scale, wd, frozen = float(g.get("lr_scale", 1.0)), float(g.get("weight_decay", weight_decay)), bool(g.get("frozen", False))
                    first = False
        out.append((s.name, s.offset, lr_scale, wd, frozen))
    for i, h in enumerate(hits):
        if h == 0:
            raise ValueError(f"param_groups[{i}]: match {param_groups[i]['match']!r} matches no parameter segment "
                             f"(names look like {', '.join(list(store.segs)[:3])}, ..., vit0.ln1.g, vp.w)")
    return out


def param_group_table(store, param_groups, weight_decay: float = 0.0) -> List[Tuple[int, int, float, float, bool]]:
    """Merged runs [(begin, end, lr_scale, wd, frozen)] of the flat parameter buffer under `param_groups` (Trainer's argument): they
    cover [0, store.numel) without gaps, in order; a segment's alignment padding goes with the segment in front of it, adjacent runs
    with equal settings are one run, boundaries are multiples of ParamStore's alignment (64 elements).  A frozen run reports
    lr_scale = wd = 0 — nothing of a frozen group's settings is ever used — so neighbouring frozen groups merge.  Host only: a
    `ParamStore(allocate=False)` is enough."""
    segs = _segment_groups(store, param_groups, weight_decay)
    runs: List[Tuple[int, int, float, float, bool]] = []
    for k, (_, off, lr_scale, wd, frozen) in enumerate(segs):
        begin = 0 if k == 0 else off
        end = segs[k + 1][1] if k + 1 < len(segs) else store.numel
        key = (0.0, 0.0, True) if frozen else (lr_scale, wd, False)
        if runs and runs[-1][2:] == key:
            runs[-1] = (runs[-1][0], end) + key
        else:
            runs.append((begin, end) + key)
    return runs


class Trainer:
    """TrainState + train_step/eval_step of main.py, for one rank.

    Gradient accumulation (`accumulate_steps=N` > 1): every `train_step(batch)` call is one MICRO-step — a forward/backward pass whose
    gradient joins a running fp32 sum (`ParamStore.acc`) — and every N-th call is the optimizer step, on the mean of the N gradients:
    the step an N-rank data-parallel run takes (`lax.pmean` over N devices, then one AdamW step, main.py:698-701), up to fp32
    summation order; on W ranks that of a W * N-rank run.  `step`, the learning-rate schedule and the bias correction advance on the
    N-th call only; the weights do not change in between.  Micro-step j of rank r draws the dropout masks of virtual rank r * N + j
    (`virtual_rank_dropout_seed`).  The sum is kept where the optimizer is: per gradient bucket on the optimizer stream beside
    backward (`acc += g`, 12 B/element), and on the N-th call AdamW reads `g + acc` itself.  With several ranks nothing is exchanged on
    the first N - 1 calls; on the N-th, `g += acc` runs in front of every bucket's all-reduce.  A call that is not the N-th returns its
    micro-batch's loss and the pending step's learning rate; the N-th returns the mean loss of the N micro-batches.  A reference
    run at 8 devices x 64 images is `accumulate_steps=8` at a per-device batch of 64 on one GPU.

    Gradient clipping (`max_grad_norm=c`): `optax.chain(clip_by_global_norm(c), adamw(...))`.  The reference builds `optax.adamw` alone
    (main.py:629-635) and never reads `training_args.max_grad_norm`, so this is opt-in and the default step stays what it is.  The
    clipped quantity is the gradient AdamW consumes — the mean over ranks and micro-steps, `gscale * x` with x the summed gradient
    (`g`, or `fp32(g + acc)` on the last micro-step of an accumulation on one rank): norm = gscale * sqrt(sum x^2), and AdamW runs with
    grad_scale = gscale if norm < c (optax's strict trigger), gscale * c / norm otherwise; no special case for zero or non-finite
    norms.  The sum of squares runs per gradient bucket on the optimizer stream beside backward, in a fixed summation order (squares
    in fp32, partials added in fp64); AdamW can no longer start before the last gradient exists, so it leaves the buckets: one pass
    over the whole buffer behind backward that reads the coefficient from device memory — the host never waits for the norm.  Every
    `train_step` call that takes the optimizer step additionally returns "grad_norm", the pre-clip norm as a fresh device scalar
    (identical on all ranks by construction); `c = math.inf` measures without clipping.

    Parameter groups (`param_groups=[dict(match=..., lr_scale=1.0, weight_decay=<the Trainer's>, frozen=False), ...]`):
    `optax.multi_transform` — one `optax.adamw(lr_fn * lr_scale, weight_decay=wd)` per group with the Trainer's b1 / b2 / eps and the
    global count, `optax.set_to_zero()` for a frozen group.  The reference builds one `optax.adamw` over all leaves (main.py:629-635),
    so this is opt-in and `None` leaves the step what it is, launch for launch.  `match` is a regex string, a list of them or a
    callable over the ParamStore segment names (`vit3.qkv.w`, `dec0.ln_sa.g`, `shared`, `flb`, `vp.w`, ...), regexes applied with
    `re.fullmatch`; the first matching group wins, an unmatched segment keeps the Trainer's weight decay and scale 1; `ENCODER` and
    `NO_DECAY` are ready-made matchers.  A leaf that is not frozen takes the usual element update with lr = fp32(lr * lr_scale) and
    its group's wd; of a frozen leaf no byte of master, compute copy, m or v ever changes (lr_scale = 0 is not frozen: the moments
    move).  The returned "learning_rate" stays the base rate; checkpoints are unchanged.  The groups reach the optimizer as a table
    of merged runs (`param_group_table`) uploaded once; every optimizer pass is one `mic_adamw_groups` launch over its slice, and a
    wholly frozen slice launches nothing.  The row split of the tied embedding is off (as with clipping: its pieces wait for the end
    of backward).  With several ranks the exchange is untouched: buckets inside frozen ranges travel as they lie and are ignored.
    When every segment of `ENCODER` is frozen, backward stops at the bridge (`skip_frozen_backward=True`, the default): the ViT's
    layer backward, its weight-gradient GEMMs and the patch-embedding gradient do not run, and the gradient buffer of those segments
    holds nothing meaningful after the step.  Not combined with gemm_dtype="fp8", accumulate_steps > 1, max_grad_norm or
    emulate_comm."""

    def __init__(self, model, learning_rate_fn: Callable[[int], float], b1=0.9, b2=0.999, eps=1e-8, weight_decay=0.0,
                 label_smoothing_factor=0.0, seed: int = 42, bucket_mb: float = 64.0, group=None, compact_head: bool = True,
                 overlap_optimizer: bool = True, grad_comm_dtype=None, gemm_dtype: Optional[str] = None,
                 fp8_scaling: str = "delayed", pack_rows: bool = True, comm_cus: Optional[int] = None, emulate_comm: int = 0,
                 fp8_head: Optional[str] = None, accumulate_steps: int = 1, max_grad_norm: Optional[float] = None,
                 param_groups: Optional[List[Dict]] = None, skip_frozen_backward: bool = True):
        """pack_rows (bfloat16 mode, with compact_head): the decoder runs on the valid caption positions only (`packed_rows`);
        exact — padded positions neither carry loss nor are attended to — and ~1/3 fewer decoder rows on ragged captions at seq 64,
        nearly half at seq 128.  Any seq_len up to max_position_embeddings and any number of encoder positions: beyond one 64x64
        attention tile the tiled attention kernels take the packed rows (`ops.attn_*_packed_tiled`).  Needs
        prefix-shaped masks available on the host: a numpy / CPU `attention_mask`, or `batch["packed_rows"]` from the collate
        function; otherwise the step runs padded.  MIC_PACK_ROWS=0 switches it off.
        grad_comm_dtype: None / torch.float32 (default: the reference's fp32 `lax.pmean`, main.py:698), torch.bfloat16 (opt-in: half
        the xGMI bytes, one more rounding per rank and element) or "auto" (opt-in; `choose_comm_dtype`: fp32 where the PROJECTED
        exchange hides under backward, bf16 where it would not — a projection from byte counts, no N > 1 run backs it).  A
        non-fp32 choice is printed by every rank.
        comm_cus (data parallel): CUs the collectives hold while backward runs — the GEMM tile planner sizes its one-round
        launches for the rest (`mic_set_cu_budget`).  Default: the channel cap exported to RCCL (`configure_rccl` before
        `init_process_group`, or NCCL_MAX_NCHANNELS in the environment) when world > 1 — the budget then equals what RCCL was held to;
        0 (planner untouched) when no cap is in force.  A user-set MIC_FREE_CUS wins over both.
        emulate_comm = N (one GPU only; bench.py --emulate-comm): every bucket's exchange is replaced by a kernel holding
        `comm_cus` CUs for the projected duration of its all-reduce among N ranks — a scheduling probe, not a scaling result.
        accumulate_steps = N: micro-batches per optimizer step (class docstring).  Not combined with gemm_dtype="fp8" (the delayed
        scales and the weight re-quantisation inside the optimizer passes assume one pass per step) or with emulate_comm.
        max_grad_norm = c (a real number > 0, math.inf allowed; default None = off, the reference's step): global-norm clipping
        in front of AdamW (class docstring).  c = inf measures the norm without clipping.  Not combined with gemm_dtype="fp8" (the
        two-phase refresh of the fp8 weight copies keys on per-bucket optimizer progress) or with emulate_comm.
        param_groups (default None = one AdamW over all leaves, the reference's step): per-group learning-rate scale, weight decay
        and freezing (class docstring).  skip_frozen_backward (with param_groups only): True = a frozen image tower's backward does
        not run; False keeps the full backward (its gradients are computed and ignored)."""
        import math
        import numbers

        import torch.distributed as dist

        if param_groups is not None:
            # everything here comes before the model is touched: the argument's shape, then the combinations that are out of scope
            _check_param_groups(param_groups)
            if gemm_dtype == "fp8":
                raise ValueError("param_groups is not supported together with gemm_dtype='fp8' (out of scope: the refresh of the fp8 weight "
                                 "copies inside the optimizer passes knows nothing of frozen ranges)")
            if not isinstance(accumulate_steps, (bool, np.bool_)) and isinstance(accumulate_steps, (int, np.integer)) and accumulate_steps > 1:
                raise ValueError("param_groups is not supported together with accumulate_steps > 1 (out of scope: AdamW on g + acc has "
                                 "no grouped form)")
            if max_grad_norm is not None:
                raise ValueError("param_groups is not supported together with max_grad_norm (out of scope: the clipped AdamW pass has no "
                                 "grouped form, and the norm of a partly frozen gradient needs its own definition)")
            if emulate_comm:
                raise ValueError("param_groups is not supported together with emulate_comm (out of scope: the stand-in exchange models "
                                 "the step whose optimizer passes all run)")
        if isinstance(accumulate_steps, bool) or not isinstance(accumulate_steps, (int, np.integer)) or accumulate_steps < 1:
            raise ValueError(f"accumulate_steps must be an integer >= 1, got {accumulate_steps!r}")
        if max_grad_norm is not None:
            if (isinstance(max_grad_norm, (bool, np.bool_)) or not isinstance(max_grad_norm, numbers.Real) or math.isnan(max_grad_norm)
                    or not max_grad_norm > 0):
                raise ValueError(f"max_grad_norm must be None or a real number > 0 (math.inf allowed), got {max_grad_norm!r}")
            if emulate_comm:
                raise ValueError("max_grad_norm is not supported together with emulate_comm (out of scope: the stand-in exchange models "
                                 "the step whose optimizer runs per bucket)")
            if gemm_dtype == "fp8" or getattr(model.engine, "fp8", False):
                raise ValueError("max_grad_norm is not supported together with gemm_dtype='fp8' (out of scope: the two-phase refresh of the "
                                 "fp8 weight copies keys on per-bucket optimizer progress)")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        # (tools/accumulate_probe.py switches a live Trainer between N and 1 by writing `accumulate_steps` and `_gscale`: state derived
        # from N in this constructor beyond those two — and buffers that only need to exist — has to be added to its `mode()` too)
        self.accumulate_steps = int(accumulate_steps)
        if self.accumulate_steps > 1 and emulate_comm:
            raise ValueError("accumulate_steps > 1 is not supported together with emulate_comm (out of scope: the stand-in exchange "
                             "models one pass per optimizer step)")
        if self.accumulate_steps > 1 and (gemm_dtype == "fp8" or getattr(model.engine, "fp8", False)):
            raise ValueError("accumulate_steps > 1 is not supported together with gemm_dtype='fp8' (out of scope: the delayed-scaling state "
                             "and the weight re-quantisation inside the optimizer passes need their own design)")
        self.model, self.lr_fn = model, learning_rate_fn
        self.b1, self.b2, self.eps, self.wd, self.ls = b1, b2, eps, weight_decay, label_smoothing_factor
        self.compact_head = compact_head
        import os as _os
        self.pack_rows = bool(pack_rows) and compact_head and _os.environ.get("MIC_PACK_ROWS", "1") != "0"
        self.step = 0  # state.step
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.group = group
        self.seed = seed
        st = model.store
        # parameter groups, host side (before any device work): which group every segment belongs to, the merged runs, and whether
        # the image tower is frozen as a whole
        self._group_runs = self._groups = None
        self._encoder_frozen = False
        if param_groups is not None:
            if getattr(model.engine, "fp8", False):
                raise ValueError("param_groups is not supported together with gemm_dtype='fp8' (out of scope: the refresh of the fp8 weight "
                                 "copies inside the optimizer passes knows nothing of frozen ranges)")
            import re

            per_seg = _segment_groups(st, param_groups, weight_decay)
            self._group_runs = param_group_table(st, param_groups, weight_decay)
            enc = [frozen for (name, _, _, _, frozen) in per_seg if re.fullmatch(ENCODER, name)]
            self._encoder_frozen = bool(enc) and all(enc)
        self.skip_frozen_backward = bool(skip_frozen_backward)
        st.ensure_grads()
        st.ensure_opt_state()
        if gemm_dtype is not None:
            model.engine.set_gemm_dtype(gemm_dtype, scaling=fp8_scaling, head=fp8_head)  # fp8_head: "all" (default) | "bwd" | "0", see Engine
        self.hyper = torch.zeros(2, dtype=torch.float32, device=model.device)
        self._hyper_pin, self._hyper_ev = None, None
        emu_world = int(emulate_comm) if (self.world == 1 and model.device.type == "cuda") else 0
        eff_world = emu_world if emu_world > 1 else self.world
        if isinstance(grad_comm_dtype, str):
            if grad_comm_dtype != "auto":
                raise ValueError(f"grad_comm_dtype must be 'auto', None or a torch dtype, got {grad_comm_dtype!r}")
            grad_comm_dtype = choose_comm_dtype(eff_world, st.numel)
        self.grad_comm_dtype = grad_comm_dtype if grad_comm_dtype not in (None, torch.float32) else None
        if self.grad_comm_dtype is not None and eff_world > 1:
            import sys

            print(f"[mic_amd.Trainer] rank {self.rank}: gradient exchange in {self.grad_comm_dtype} — NOT the reference's fp32 pmean "
                  "(main.py:698); pass grad_comm_dtype=None for fp32", file=sys.stderr, flush=True)
        if comm_cus is not None:
            self.comm_cus = int(comm_cus)
        elif emu_world > 1:
            self.comm_cus = COMM_CUS_DEFAULT   # the stand-in collectives are held to exactly this many CUs by their stream's mask
        else:
            self.comm_cus = min(rccl_channel_cap(), 128) if self.world > 1 else 0
        # one-round GEMM launches are sized for the CUs the collectives leave (process-wide planner state: set for the duration of a
        # train step, see train_step); a MIC_FREE_CUS exported by the user is the user's budget and stays in force
        self._cu_budget = 256 - self.comm_cus if (model.device.type == "cuda" and eff_world > 1 and self.comm_cus > 0
                                                  and not _os.environ.get("MIC_FREE_CUS")) else 0
        self.buckets = bucket_plan(st, bucket_mb)
        cb = 2 if self.grad_comm_dtype in (torch.bfloat16, torch.float16) else 4
        if eff_world > 1 and self.rank == 0:
            import sys

            desc = describe_buckets(st, self.buckets, cb)
            total = sum(d["MB"] for d in desc)
            print(f"[mic_amd.Trainer] data parallel over {eff_world} ranks{' (EMULATED on one GPU)' if emu_world > 1 else ''}: {len(desc)} gradient "
                  f"buckets in backward-completion order, {total:.0f} MB per exchange in {'bf16' if cb == 2 else 'fp32'} (all-reduce, projected "
                  f"{allreduce_ms(total * 1e6, eff_world):.1f} ms over xGMI against ~{BACKWARD_WINDOW_MS:.0f} ms of backward); "
                  + (f"RCCL capped at {self.comm_cus} channels, GEMM tile planner sized for {256 - self.comm_cus} CUs" if self._cu_budget else
                     "no RCCL channel cap in force (mic_amd.train.configure_rccl before init_process_group), GEMM tile planner sized for all CUs")
                  + f"; first: {desc[0]['first']}..{desc[0]['last']} {desc[0]['MB']:.0f} MB, last: {desc[-1]['first']}..{desc[-1]['last']} "
                  f"{desc[-1]['MB']:.0f} MB; sizes MB {[d['MB'] for d in desc]}", file=sys.stderr, flush=True)
        # MIC_OPT_OVERLAP=0: AdamW as one launch after backward (profiling aid: per-bucket AdamW on its own stream shares HBM with
        # the backward kernels it overlaps, so their individual durations read longer than the kernels are)
        import os

        if os.environ.get("MIC_OPT_OVERLAP", "1") == "0":
            overlap_optimizer = False
        self.overlap_optimizer = overlap_optimizer
        sh = st.segs["shared"]
        # The tied embedding's gradient is complete only at the end of backward (its sparse input-embedding rows): AdamW runs
        # early on every row this step's decoder ids do not touch and late on the <= world*B*T rows they do (`_adamw_slice` /
        # `_adamw_shared_late`; MIC_OPT_SPLIT_SHARED=0: the whole segment waits for the end).  MIC_OPT_CUS: CUs of the optimizer
        # stream's mask.
        # Clipping (max_grad_norm): AdamW cannot start before the last gradient exists, so the optimizer leaves the buckets — the row
        # split only serves the early passes and is off; what runs per bucket beside backward is the bucket's sum of squares.
        # Parameter groups: the row split is off as well — there are no group-aware row passes; the pieces of the tied embedding wait for
        # the end of backward, every other bucket's grouped pass still runs beside it.
        clip = self.max_grad_norm is not None
        grouped = self._group_runs is not None
        self._split_shared = (self.overlap_optimizer and model.device.type == "cuda" and not clip and not grouped
                              and _os.environ.get("MIC_OPT_SPLIT_SHARED", "1") != "0" and sh.numel % st.d == 0)
        self._sh = (sh.offset, sh.offset + sh.numel, st.d)
        self._row_flag = torch.zeros(sh.numel // st.d, dtype=torch.uint8, device=model.device) if self._split_shared else None
        opt_cus = (int(_os.environ.get("MIC_OPT_CUS", str(OPT_CUS_DEFAULT)))
                   if (model.device.type == "cuda" and (self._split_shared or ((clip or grouped) and self.overlap_optimizer))) else 0)
        # (tools/param_groups_probe.py switches a live Trainer between the grouped forms and the plain step by writing `_groups`,
        # `_group_runs`, `_encoder_frozen`, `skip_frozen_backward`, `_split_shared`, `_row_flag` and the reducer's `ready_when`: state
        # derived from param_groups beyond those has to be added to its `mode()` too)
        if grouped:
            self._groups = ops.AdamwRuns(self._group_runs, model.device)  # the device table: made once, read by every grouped pass
        import weakref

        me = weakref.ref(self)  # the reducer's callbacks must not own the Trainer (Trainer -> reducer -> bound method -> Trainer is a cycle
        #                         that keeps ~16 GB of device state alive after `del trainer, model` until the cycle collector runs)
        # the pieces of the tied embedding: "next" (the head's dX GEMM, issued right behind the dE GEMM that completes the dense
        # half of the gradient, still reads the weights) when the row split is on, "end" otherwise
        gate = "next" if self._split_shared else "end"
        when = [gate if (b < sh.offset + sh.numel and e > sh.offset) else "exchanged" for (b, e) in self.buckets]
        # (clipping: `gate` is "end" — the pieces of the tied embedding receive the sparse input-embedding rows late, with several ranks
        # only inside finish(before=_scatter_embedding_rows) — and every other bucket's sum of squares runs right behind its exchange)
        on_ready = (lambda b, e: me()._sumsq_slice(b, e)) if clip else (lambda b, e: me()._adamw_slice(b, e))
        self.reducer = GradReducer(st.grad, self.buckets, group, on_ready=on_ready if self.overlap_optimizer else None,
                                   ready_when=when, comm_dtype=self.grad_comm_dtype, opt_cus=opt_cus,
                                   emulate=dict(world=emu_world, cus=self.comm_cus or COMM_CUS_DEFAULT, comm_bytes=cb) if emu_world > 1 else None)
        self.metrics_buf = torch.zeros(2, dtype=torch.float32, device=model.device)
        self._pos = {}
        self._det_ws = None  # workspace of the deterministic embedding-row scatter (data parallel)
        self._late_done = False
        self._late_early = _os.environ.get("MIC_LATE_EARLY", "1") != "0"  # (A/B: 0 = the flagged embedding rows' pass behind the step, as before)
        # pmean(grad): SUM in the flat buffer, the mean folded into AdamW's grad_scale (over the ranks and, with accumulation, the micro-steps)
        self._gscale = 1.0 / self.world
        self._use_acc = False  # True while the optimizer passes of an accumulation's last micro-step are issued (world 1: AdamW on g + acc)
        self._micro = 0        # micro-steps taken since the last optimizer step
        self._loss_sum = None  # accumulation: the sum of their losses (device scalar)
        if self.accumulate_steps > 1:
            st.ensure_grad_acc()
            self._gscale = 1.0 / (self.world * self.accumulate_steps)
            # a micro-step that only accumulates: the pieces of the tied embedding wait for the input-embedding scatter at the end of
            # decoder backward ("end"); every other bucket joins the sum as soon as backward reports it
            self._when_acc = ["end" if (b < sh.offset + sh.numel and e > sh.offset) else "exchanged" for (b, e) in self.buckets]
            self._acc_cb = lambda b, e: me()._accumulate_slice(b, e)
            self._pre_cb = lambda b, e: me()._add_acc_slice(b, e)
        # clipping: one slot range per bucket in a partials buffer (laid out once, from the kernel's own launch geometry), or the slots
        # of ONE pass over the whole buffer when nothing runs per bucket; (norm, coef) of the step.  None without max_grad_norm.
        # (tools/clip_probe.py switches a live Trainer between the clipped and the plain step by writing `_clip_out`, `_split_shared`,
        # `_row_flag` and the reducer's `on_ready` / `ready_when`: state derived from max_grad_norm beyond those has to be added to its
        # `mode()` too)
        self._clip_partials = self._clip_out = None
        if clip:
            self._clip_off, n_slots = {}, 0
            for (b, e) in (self.buckets if self.reducer.on_ready is not None else [(0, st.numel)]):
                self._clip_off[b] = n_slots
                n_slots += ops.grad_sumsq_slots(e - b)
            self._clip_slots = n_slots
            self._clip_partials = torch.empty(n_slots, dtype=torch.float32, device=model.device)
            self._clip_out = torch.empty(2, dtype=torch.float32, device=model.device)

    def _sumsq_slice(self, b: int, e: int):
        """clipping: the sum of squares of flat slice [b, e) of the gradient AdamW will consume (g, or g + acc on the last micro-step of
        an accumulation on one rank) into the slice's own range of the partials buffer — on the reducer's side stream, beside backward"""
        st = self.model.store
        off = self._clip_off[b]
        ops.grad_sumsq(st.grad[b:e], self._clip_partials[off:], acc=st.acc[b:e] if self._use_acc else None, n=e - b)

    def _clipped_adamw(self, per_bucket: bool):
        """clipping, behind finish() on the step's own stream: (norm, coef) from all slots, then ONE AdamW over the whole buffer that
        reads coef from the device"""
        st = self.model.store
        acc = st.acc if self._use_acc else None
        if not per_bucket:
            ops.grad_sumsq(st.grad, self._clip_partials, acc=acc)
        ops.clip_coef(self._clip_partials, self._clip_slots, self._gscale, self.max_grad_norm, self._clip_out)
        ops.adamw_clip(st.master, st.m, st.v, st.grad, None if st.lp is st.master else st.lp, self.hyper, self._clip_out[1:2], self.b1,
                       self.b2, self.eps, self.wd, acc=acc)

    def _adamw_slice(self, b: int, e: int):
        """AdamW on flat slice [b, e) — runs on the reducer's side stream right after that bucket's all-reduce.  The part of the
        slice inside the tied embedding (whole rows: the bucket cuts inside that segment are row-aligned) skips the rows flagged
        for this step when the row split is on (`_adamw_shared_late` takes those)."""
        st = self.model.store
        if self._groups is not None:  # parameter groups: one launch whatever runs the slice crosses, none if all of them are frozen
            ops.adamw_groups(self._groups, b, st.master[b:e], st.m[b:e], st.v[b:e], st.grad[b:e], None if st.lp is st.master else st.lp[b:e],
                             self.hyper, self.b1, self.b2, self.eps, grad_scale=self._gscale, n=e - b)
            return
        sb, se, width = self._sh
        lo, hi = max(b, sb), min(e, se)
        if not self._split_shared or lo >= hi:
            ops.adamw(st.master[b:e], st.m[b:e], st.v[b:e], st.grad[b:e], None if st.lp is st.master else st.lp[b:e], self.hyper,
                      self.b1, self.b2, self.eps, self.wd, grad_scale=self._gscale, n=e - b, acc=st.acc[b:e] if self._use_acc else None)
            return
        assert (lo - sb) % width == 0 and (hi - sb) % width == 0, "bucket cuts inside the tied embedding are row-aligned"
        for (x, y) in ((b, lo), (hi, e)):
            if y > x:
                ops.adamw(st.master[x:y], st.m[x:y], st.v[x:y], st.grad[x:y], None if st.lp is st.master else st.lp[x:y], self.hyper,
                          self.b1, self.b2, self.eps, self.wd, grad_scale=self._gscale, n=y - x, acc=st.acc[x:y] if self._use_acc else None)
        self._adamw_shared(0, (lo - sb) // width, (hi - sb) // width)

    def _adamw_shared(self, want: int, r0: int = 0, r1: Optional[int] = None):
        """AdamW on rows [r0, r1) of the tied embedding whose flag equals `want`"""
        st = self.model.store
        sb, se, width = self._sh
        r1 = (se - sb) // width if r1 is None else r1
        x, y = sb + r0 * width, sb + r1 * width
        ops.adamw_rows(r1 - r0, width, self._row_flag[r0:r1], want, st.master[x:y], st.m[x:y], st.v[x:y], st.grad[x:y],
                       None if st.lp is st.master else st.lp[x:y], self.hyper, self.b1, self.b2, self.eps, self.wd,
                       grad_scale=self._gscale, acc=st.acc[x:y] if self._use_acc else None)

    def _accumulate_slice(self, b: int, e: int):
        """a micro-step that is not the last: acc[b:e] = grad[b:e] (first micro-step) or += (the following), on the reducer's side stream"""
        st = self.model.store
        ops.grad_accumulate(st.acc[b:e], st.grad[b:e], init=self._micro == 0, n=e - b)

    def _add_acc_slice(self, b: int, e: int):
        """last micro-step, several ranks: grad[b:e] += acc[b:e] on the collective stream, in front of the bucket's all-reduce"""
        st = self.model.store
        ops.grad_accumulate(st.grad[b:e], st.acc[b:e], init=False, n=e - b)

    def _adamw_shared_late(self):
        """end of backward (after the sparse embedding rows have been added): the flagged rows of the tied embedding"""
        self._adamw_shared(1)

    def _embed_rows_done(self):
        """engine hook (world 1): the late pass of the tied embedding on the optimizer stream, behind everything enqueued so far"""
        r = self.reducer
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(r.opt_stream):
            r.opt_stream.wait_event(ev)
            with ops.pinned_stream():
                self._adamw_shared_late()
            ev2 = torch.cuda.Event()
            ev2.record(r.opt_stream)
        self._late_done = True
        # fp8 GEMMs: the weights whose optimizer passes are on the optimizer stream by now (the decoder's) become fp8 for the next step
        # here, under the ViT's backward
        if r.next > 0:
            # ... up to the first bucket whose optimizer pass has been released but not ISSUED yet ("next" buckets wait for the following
            # progress report, "end" buckets for finish()): its weights are not final behind `ev2`
            upto = r.buckets[r.next - 1][1]
            for held in (r._pending, r._at_end):
                if held:
                    upto = min(upto, min(h[0] for h in held))
            if upto > 0 and self.model.engine.f8 is not None:
                self.model.engine.f8.refresh_weights(ops.role_stream(self.model.device, "aux"), upto=upto, wait_event=ev2)

    def _flag_embedding_rows(self, ids: torch.Tensor):
        """flags the rows of `shared` that this step's decoder input ids (of every rank) will add a sparse gradient to"""
        if self.world > 1:
            import torch.distributed as dist

            all_ids = torch.empty((self.world * ids.numel(),), dtype=ids.dtype, device=ids.device)
            dist.all_gather_into_tensor(all_ids, ids.contiguous(), group=self.group)
            ids = all_ids
        ops.row_flags(ids, ids.numel(), self._row_flag)

    def _scatter_embedding_rows(self):
        """Data parallel: the sparse half of the tied-embedding gradient.  Every rank all-gathers (ids, dh0) — <= B*T rows
        per rank — and adds ALL ranks' rows into its already all-reduced dense half (sum over ranks, like the all-reduce; 1/world
        is applied by AdamW) with the DETERMINISTIC scatter: the same bits on every rank, so the replicas' embeddings stay
        identical (the atomics of the single-process scatter do not guarantee an order).  Runs after the last collective."""
        import torch.distributed as dist

        eng, st = self.model.engine, self.model.store
        ids, dh0, M = eng.embed_rows
        all_ids = torch.empty((self.world * M,), dtype=ids.dtype, device=ids.device)
        all_dh = torch.empty((self.world * M, st.d), dtype=dh0.dtype, device=dh0.device)
        dist.all_gather_into_tensor(all_ids, ids[:M].contiguous(), group=self.group)
        dist.all_gather_into_tensor(all_dh, dh0[:M].contiguous(), group=self.group)
        if self._det_ws is None:
            self._det_ws = ops.embed_rows_add_det_workspace(st.g("shared").numel() // st.d, all_ids.device)
        ops.embed_rows_add_det(all_ids, all_dh, eng.embed_scale, st.g("shared").view(-1, st.d), self.world * M, st.d, self._det_ws)

    def _prep(self, batch):
        m = self.model
        # several captions per image: G caption rows per image, image-major (refusals come before any device work)
        G = check_captions_per_image(batch, bool(getattr(m.engine, "fp8", False)))
        self._images = int(batch["pixel_values"].shape[0]) if G > 1 else None
        lw = check_loss_weights(batch, bool(getattr(m.engine, "fp8", False)))
        px = m._dev(batch["pixel_values"], torch.float32)
        labels = m._dev(batch["input_ids"], torch.int32)
        mask = m._dev(batch["attention_mask"], torch.int32)
        dec_in = m._dev(batch["decoder_input_ids"], torch.int32)
        B, T = labels.shape
        pos = self._pos.get((B, T))  # position ids 0 .. T-1 per sequence: built once per batch shape (two launches per step otherwise)
        if pos is None:
            pos = self._pos[(B, T)] = torch.arange(T, dtype=torch.int32, device=m.device)[None].expand(B, T).contiguous()
        rows = row_labels = None
        pk = batch.get("packed_rows") if self.pack_rows else None
        if self.compact_head:
            if "loss_rows" in batch:  # precomputed by the collate function (no device->host sync in the step)
                idx, rl = batch["loss_rows"]
                idx, rl = m._dev(idx, torch.int32), m._dev(rl, torch.int32)
            else:
                am = batch["attention_mask"]
                am = am.cpu().numpy() if isinstance(am, torch.Tensor) else np.asarray(am)
                lb = batch["input_ids"]
                lb = lb.cpu().numpy() if isinstance(lb, torch.Tensor) else np.asarray(lb)
                idx, rl = loss_rows(am, lb)
                idx, rl = m._dev(idx, torch.int32), m._dev(rl, torch.int32)
                if self.pack_rows and pk is None:
                    di = batch["decoder_input_ids"]
                    pk = packed_rows(am, di.cpu().numpy() if isinstance(di, torch.Tensor) else np.asarray(di))
            if 0 < idx.numel() < B * T:
                rows, row_labels = (idx, int(idx.numel())), rl
        # packed decoder rows: bf16-storage kernels, compacted head on the same rows (any seq_len, any number of encoder positions)
        self._pack = None
        eng = m.engine
        if pk is not None and rows is not None and eng.dt == torch.bfloat16:
            ql = pk[1]
            if not (isinstance(ql, torch.Tensor) and ql.is_cuda):
                # host-side description: it must describe the same positions as `loss_rows` (a collate function that built the two
                # from different masks would make the attention kernels index rows the LM head does not own).  Device-resident
                # descriptions are trusted: checking them would put a device-to-host sync into every step.
                n_pk = int(np.asarray(ql).sum()) if not isinstance(ql, torch.Tensor) else int(ql.sum())
                if n_pk != rows[1]:
                    raise ValueError(f"batch['packed_rows'] describes {n_pk} decoder rows but batch['loss_rows'] has {rows[1]}: both must come from the same attention_mask")
            grouped = ()
            if G > 1:
                # the cross-attention beyond one tile takes an image's captions as one sequence: its description, from the host copies
                host = [t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in pk[:2]]
                grouped = tuple(m._dev(t, torch.int32) for t in group_packed_rows(host[0], host[1], G))
            q_off, q_len, ids_p, pos_p = (m._dev(t, torch.int32) for t in pk)
            self._pack = ((q_off, q_len, rows[1]) + grouped, ids_p, pos_p)
        self._rows, self._row_labels = rows, row_labels
        # per-caption / per-token loss weights -> one fp32 weight per head row: broadcast over T, gathered at the compacted head's rows
        # (fresh tensors, fully written: nothing kept from an earlier step)
        self._loss_kw = {}
        if lw is not None:
            w = m._dev(lw, torch.float32)
            w = (w[:, None].expand(B, T) if w.dim() == 1 else w).reshape(-1)
            self._loss_kw = dict(row_weights=torch.index_select(w, 0, rows[0]) if rows is not None else w.contiguous())
        return px, labels, mask, dec_in, pos, B, T

    def _set_hyper(self, lr: float, count: float) -> None:
        """(lr, bias-correction count) of this step into the device pair AdamW reads.  From PINNED host memory: a host-to-device
        copy out of pageable memory is carried out by the runtime synchronously behind everything queued on the stream, i.e.
        it was a full device sync per step (the host could not queue step k+1 under step k)."""
        if self.hyper.device.type != "cuda":
            self.hyper.copy_(torch.tensor([lr, count], dtype=torch.float32))
            return
        if self._hyper_pin is None:
            self._hyper_pin = torch.empty((8, 2), dtype=torch.float32).pin_memory()
            self._hyper_ev = [None] * 8
        slot = self.step % 8
        if self._hyper_ev[slot] is not None:
            self._hyper_ev[slot].synchronize()  # the copy that last read this slot (8 steps ago) has run
        self._hyper_pin[slot, 0] = lr
        self._hyper_pin[slot, 1] = count
        self.hyper.copy_(self._hyper_pin[slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hyper_ev[slot] = ev

    def train_step(self, batch: Dict) -> Dict[str, float]:
        """main.py:684-707.  batch["captions_per_image"] = G (optional, an int >= 1): `pixel_values` holds n_img images, the caption
        tensors (and "loss_rows" / "packed_rows") n_img * G rows, image-major — caption row r belongs to image r // G.  The step is the
        one on pixel_values.repeat_interleave(G, 0) with the image tower and the cross k/v projections run once per image; refused
        (ValueError, before any device work): a G that is no int >= 1, caption rows != n_img * G, G > 1 with fp8 GEMMs.
        batch["loss_weights"] = w (optional; fp32 [R] per caption row or [R, T] per token, a host array or a device tensor; any finite
        value, zeros and negatives included): loss = sum_{r,t} w[r,t] m[r,t] l[r,t] / sum_{r,t} m[r,t] with m the attention mask and
        l the per-token loss (label smoothing included), and the gradients of that loss; "loss" in the metrics is this weighted loss.
        The denominator is the number of valid tokens whatever w is — advantages may sum to zero, and a caption with w = 0 still counts
        there (the mask drops it).  All weights 1.0 give the plain step bit for bit; without the key it is the plain step launch for
        launch.  Refused (ValueError, before any device work): a shape other than [R] / [R, T], non-finite values in a host array (a
        device tensor's values are trusted), fp8 GEMMs."""
        # (a micro-step that only accumulates issues no collective: the planner keeps all CUs there)
        budget = self._cu_budget if not (self.accumulate_steps > 1 and self._micro < self.accumulate_steps - 1) else 0
        if budget:
            ops.set_cu_budget(budget)
        try:
            ms = self.reducer.step_stream
            if ms is None:
                return self._step(batch)
            # the optimizer's stream carries a CU mask, which makes it a blocking stream: the step keeps off the null stream
            cur = torch.cuda.current_stream()
            ms.wait_stream(cur)
            with torch.cuda.stream(ms):
                out = self._step(batch)
            cur.wait_stream(ms)
            return out
        finally:
            if budget:
                ops.set_cu_budget(0)  # generation / evaluation have no collective beside them

    def _step(self, batch: Dict) -> Dict[str, float]:
        """One `train_step` call = micro-step j = self._micro of the pending optimizer step under accumulate_steps = N (N = 1: the step
        itself).  j < N - 1: backward into `grad`, then `acc (+)= grad` — per bucket on the optimizer stream as backward reports it, no
        exchange, no optimizer, the weights untouched.  j = N - 1: the optimizer step (main.py:684-707), for N > 1 on grad + acc, with
        grad_scale 1 / (world * N)."""
        m, st, eng = self.model, self.model.store, self.model.engine
        N, j = self.accumulate_steps, self._micro
        final = j == N - 1
        px, labels, mask, dec_in, pos, B, T = self._prep(batch)
        seed = virtual_rank_dropout_seed(self.seed, self.rank, self.step, N, j)  # split(dropout_rng) per step (main.py:686)
        if j == 0:
            # (lr, count) of the pending optimizer step — the schedule at the pre-increment count, bias correction with count+1 (SURVEY
            # B10): AdamW reads them on the last micro-step, the metrics on every one
            self._set_hyper(float(self.lr_fn(self.step)), float(self.step + 1))
        r = self.reducer
        per_bucket = r.on_ready is not None
        if final:
            # accumulation, one rank: every AdamW launch reads g + acc.  Several: the sum joins the gradient in front of each all-reduce,
            # AdamW is the plain one
            self._use_acc = N > 1 and self.world == 1
            r.start_step(pre_exchange=self._pre_cb if (N > 1 and self.world > 1) else None)
        else:
            r.start_step(local=True, on_ready=self._acc_cb if per_bucket else None, ready_when=self._when_acc)
        eng.grad_progress = r.progress if r.active else None
        # the sparse input-embedding rows: scattered locally while accumulating (acc carries them), exchanged on the last micro-step
        eng.defer_embed = final and self.world > 1
        # a frozen image tower: backward stops at the bridge (Engine.loss_and_grads)
        eng.skip_vit_backward = self._encoder_frozen and self.skip_frozen_backward
        # single process: the flagged rows of the tied embedding get their optimizer pass as soon as decoder backward has scattered the
        # input-embedding rows into them — under the ViT's backward instead of behind the step (0.09 ms + a stream hand-over)
        self._late_done = False
        eng.on_embed_rows = self._embed_rows_done if (final and self.world == 1 and self._split_shared and per_bucket
                                                      and self._late_early) else None
        try:
            with ops.pinned_stream():
                if final and self._split_shared:  # (accumulation: the rows of THIS micro-step's ids only — acc is already complete for every row)
                    self._flag_embedding_rows(self._pack[1] if self._pack is not None else dec_in.reshape(-1))
                if self._pack is not None:  # the decoder sees the valid positions only
                    pack, ids_p, pos_p = self._pack
                    loss = eng.loss_and_grads(px, ids_p, pos_p, None, labels.reshape(-1), B, T, label_smoothing=self.ls, seed=seed,
                                              rows=self._rows, row_labels=self._row_labels, pack=pack, images=self._images, **self._loss_kw)
                else:
                    loss = eng.loss_and_grads(px, dec_in.reshape(-1), pos.reshape(-1), mask, labels.reshape(-1), B, T,
                                              label_smoothing=self.ls, seed=seed, rows=self._rows, row_labels=self._row_labels,
                                              images=self._images, **self._loss_kw)
            eng.on_embed_rows = None
            if not final:
                r.finish()
                if not per_bucket:  # overlap_optimizer=False: one pass over the whole buffer behind backward, like its AdamW
                    ops.grad_accumulate(st.acc, st.grad, init=j == 0)
                self._loss_sum = loss.reshape(1).clone() if j == 0 else self._loss_sum + loss.reshape(1)
                self._micro = j + 1
                out = torch.cat((loss.reshape(1), self.hyper[0:1]))
                return {"loss": out[0], "learning_rate": out[1]}
            # pmean(grad) (main.py:698): SUM here, 1/world folded into AdamW's grad_scale.  The remaining buckets go out; behind them the
            # sparse embedding-row exchange, the optimizer passes that had to wait for it, and the flagged rows of the tied embedding
            r.finish(before=self._scatter_embedding_rows if self.world > 1 else None,
                     after=self._adamw_shared_late if (self._split_shared and not self._late_done) else None)
            if self._clip_out is not None:
                self._clipped_adamw(per_bucket)
            elif not self.overlap_optimizer and self._groups is not None:
                self._adamw_slice(0, st.numel)
            elif not self.overlap_optimizer:
                ops.adamw(st.master, st.m, st.v, st.grad, None if st.lp is st.master else st.lp, self.hyper, self.b1, self.b2, self.eps,
                          self.wd, grad_scale=self._gscale, acc=st.acc if self._use_acc else None)
            m.invalidate_params_cache(by_optimizer=True)
            if m.device.type == "cuda":
                aux = ops.role_stream(m.device, "aux")
                if eng.f8 is not None:
                    eng.f8.refresh_weights(aux)  # fp8 GEMMs: next step's weight copies, beside the glue between the steps
                # the k-contiguous copy of the tied embedding for the NEXT step's head backward: behind this step's optimizer passes, on a
                # stream of its own — it has the whole next forward pass to finish (engine.shared_T waits for it)
                eng.refresh_shared_T(aux, st.version)
        except BaseException:
            # a step that raised: some optimizer passes may have run — master and compute copy have moved, so everything derived from them
            # (model.params, E^T, the LayerNorm folds, vocabulary shortlists: ParamStore.version) is stale; a refresh of the fp8 weight
            # copies may be under way — the next pass waits for it and re-makes them all from the weights as they are, their scale
            # history restarted (Fp8State)
            m.invalidate_params_cache()
            raise
        finally:
            eng.skip_vit_backward = False
            eng.on_embed_rows, eng.grad_progress, self._use_acc = None, None, False  # (whatever happened: no hooks into this Trainer stay behind)
        self.step += 1
        self._micro = 0
        # accumulation: the reference's pmean'd loss over the N virtual ranks; stays on the device
        mean = loss.reshape(1) if N == 1 else (self._loss_sum + loss.reshape(1)) * (1.0 / N)
        self._loss_sum = None
        if self.world == 1:
            # one launch instead of three (two copies + a clone) in the gap between two steps; fresh storage per step (callers keep these)
            if self._clip_out is not None:
                out = torch.cat((mean, self.hyper[0:1], self._clip_out[0:1]))
                return {"loss": out[0], "learning_rate": out[1], "grad_norm": out[2]}
            out = torch.cat((mean, self.hyper[0:1]))
            return {"loss": out[0], "learning_rate": out[1]}
        self.metrics_buf[0:1].copy_(mean)
        self.metrics_buf[1:2].copy_(self.hyper[0:1])  # lr, device to device (a Python scalar assigned into a device tensor syncs)
        out = self._pmean_metrics()
        if self._clip_out is not None:
            # the pre-clip norm: every rank summed the same all-reduced bytes in the same order, so it needs no pmean
            out["grad_norm"] = self._clip_out[0].clone()
        return out

    def eval_step(self, batch: Dict) -> Dict[str, float]:
        """main.py:710-721 (train=False, no dropout).  batch["loss_weights"]: the weighted loss of train_step."""
        m, eng = self.model, self.model.engine
        px, labels, mask, dec_in, pos, B, T = self._prep(batch)
        if self._pack is not None:
            pack, ids_p, pos_p = self._pack
            loss = eng.loss_only(px, ids_p, pos_p, None, labels.reshape(-1), B, T, label_smoothing=self.ls, rows=self._rows,
                                 row_labels=self._row_labels, pack=pack, images=self._images, **self._loss_kw)
        else:
            loss = eng.loss_only(px, dec_in.reshape(-1), pos.reshape(-1), mask, labels.reshape(-1), B, T, label_smoothing=self.ls,
                                 rows=self._rows, row_labels=self._row_labels, images=self._images, **self._loss_kw)
        self.metrics_buf[0:1].copy_(loss)
        self.metrics_buf[1:2].zero_()
        out = self._pmean_metrics()
        out.pop("learning_rate")
        return out

    # ------------------------------------------------------------------ checkpoints (main.py:299-345)
    def save_checkpoint(self, save_dir: str, with_opt: bool = False, overwrite: bool = False) -> str:
        """`save_model_checkpoint`: `<save_dir>/ckpt-<step-1>/` with config.json + flax_model.msgpack, and with
        `with_opt` also opt_state.msgpack + training_state.json.  Rank 0 writes (state is replicated, main.py:300)."""
        import os

        from .checkpoint import save_train_state

        if self._micro != 0:
            raise RuntimeError(f"save_checkpoint in the middle of a gradient accumulation ({self._micro} of {self.accumulate_steps} micro-steps "
                               "taken): the running gradient sum is not part of a checkpoint; save after the optimizer step")
        ckpt = os.path.join(save_dir, f"ckpt-{self.step - 1}")
        if self.rank != 0 or (os.path.exists(ckpt) and not overwrite):  # main.py:304-305
            return ckpt
        torch.cuda.synchronize(self.model.device) if self.model.device.type == "cuda" else None
        self.model.save_pretrained(ckpt)
        if with_opt:
            save_train_state(ckpt, self.model.store, self.step)
        return ckpt

    def restore_checkpoint(self, ckpt_dir: str) -> int:
        """`restore_model_checkpoint` (main.py:330-345) — applied to this trainer (the reference's `state.replace` line is
        commented out, 345): parameters, AdamW moments, step counter.  Returns the restored step."""
        from .checkpoint import load_train_state

        self.step = load_train_state(ckpt_dir, self.model.store)
        self._micro = 0  # a pending accumulation belongs to the state that was replaced
        self.model.invalidate_params_cache()
        return self.step

    def _pmean_metrics(self) -> Dict[str, torch.Tensor]:
        """pmean of the 2 scalars (main.py:703-704, 719).  Returned as device tensors (no host sync in the step)."""
        if self.world > 1:
            import torch.distributed as dist

            dist.all_reduce(self.metrics_buf, op=dist.ReduceOp.SUM, group=self.group)
            self.metrics_buf /= self.world
        out = self.metrics_buf.clone()  # fresh storage per step: callers keep these around (main.py:776 `train_metrics.append`)
        return {"loss": out[0], "learning_rate": out[1]}
