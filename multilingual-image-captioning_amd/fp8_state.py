"""State of the fp8 GEMM operands (BASELINE configs[4]): the e4m3 weight copies and their once-per-step refresh, the scale slots of
the quantised activations / gradients, and the fp8 inputs the forward pass keeps for the weight-gradient GEMMs.  `Engine` owns one
`Fp8State` (`Engine.f8`) while its projections run as fp8 GEMMs and none otherwise; activation buffers come from `Engine.buf`."""
from __future__ import annotations

import os
from typing import Dict, NamedTuple, Optional

import torch

from . import ops
from .params import _rup

E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


class Q8(NamedTuple):
    """a quantised tensor: its fp8 bytes and its scale slot, fp32 [2] = (amax, 1 / scale)"""
    q: torch.Tensor
    state: torch.Tensor

    @property
    def scale_inv(self):
        return self.state[1:]


class W8(NamedTuple):
    """the fp8 copies of a weight: q [out][in] (forward: x W^T), qT [in][out] (dX = dy W), one scale slot"""
    q: torch.Tensor
    qT: torch.Tensor
    state: torch.Tensor

    @property
    def scale_inv(self):
        return self.state[1:]


class Q8Target(NamedTuple):
    """a tensor its PRODUCER emits as fp8 bytes (`Fp8State.target`): `out` is the descriptor the LayerNorm / attention kernels take,
    `c_q8` = (state, partials) the one a GEMM epilogue takes"""
    q: torch.Tensor
    state: torch.Tensor
    out: object
    c_q8: tuple

    @property
    def q8(self) -> Q8:
        return Q8(self.q, self.state)

    def view(self, q: torch.Tensor) -> "Q8Target":
        """the same tensor (scale slot, partial maxima) seen through the column slice `q` of its bytes"""
        return Q8Target(q, self.state, ops.fp8_out(q, self.state, self.c_q8[1]), self.c_q8)


class Fp8Views:
    """read-only views on `Engine` of what callers outside the package read there: `fp8_fused` and `_a8_ready` whatever the GEMM
    mode, the weight copies and the activation slots (tests hold them against a reference quantiser) in the fp8 mode"""

    @property
    def fp8_fused(self) -> bool:
        return self.f8 is not None and self.f8.fused

    @property
    def _a8_ready(self) -> set:
        return self.f8.ready if self.f8 is not None else set()

    _w8 = property(lambda self: self.f8.weights)
    _a8_slots = property(lambda self: self.f8.slots)
    _a8_part = property(lambda self: self.f8.a_part)


IDLE, ROLLED, COMPLETE = "idle", "rolled", "complete"


class Fp8State:
    """Weights.  `weights[name]` holds the copies the fp8 GEMMs read; `stale` says the bf16 weights moved since they were made
    (`weights_changed`), `seen` that the scale slots carry the amax the previous quantiser pass recorded (delayed scaling).  Stale
    copies are re-made at the start of the next pass (`begin_pass`) — unless the Trainer had them made before, on a side stream behind
    the optimizer (delayed scaling, MIC_FP8_W8_ASYNC): two `refresh_weights` calls per step, whose progress is `phase`:

        call                                    phase before -> after   stream
        refresh_weights(side, upto, ev)         idle -> rolled          side, behind `ev` (optimizer stream): roll the amax, the
          end of decoder backward                                       weights below `upto` (the decoder's), under ViT backward
        refresh_weights(side)                   idle | rolled           side, behind the step's stream: roll unless rolled, the
          end of the step                         -> complete           other weights; records the event `pending`
        wait()                                  complete -> idle        the caller's: waits for `pending`
          first fp8 GEMM of the next pass
        begin_pass()                            rolled -> idle          the caller's: waits for the side stream (only a step that
          start of every pass                                           ended between the two calls leaves "rolled" behind)

    `pending` is never dropped unwaited: whoever writes the copies next (`begin_pass` with stale weights) or reads them waits first.
    Nothing else resets a phase; `weights_changed()` (not by the optimizer: params setter, checkpoint restore, a step that raised)
    makes the next pass wait, restart the scale history from the current amax and re-quantise everything.

    Activations / gradients.  One (amax, 1 / scale) slot per tensor tag, + its partial maxima under delayed scaling; `ready`: the
    tags whose slot carries the previous pass's amax — those are quantised in one pass (`quant`) or, `fused`, emitted by their
    producer (`target`).  `saved`, `head_x`, `head_dy`: what backward reads of this pass's forward."""

    KINDS = ("qkv", "cq", "ckv", "fc1", "fc2")  # the QKV and FFN projections of both towers; out-projections stay bf16

    def __init__(self, store, buf, rowpad: int, scaling: str, head: Optional[str], ckv_hoist: bool, ln_partials: bool):
        P = self.P = store
        self.buf, self.rowpad, self.scaling, dev = buf, rowpad, scaling, store.device
        self.delayed = scaling == "delayed"
        # the cross-attention k/v projections of all layers as ONE fp8 matrix "ckvcat" (one scale) when they run hoisted (ckv_hoisted)
        kinds = tuple(k for k in self.KINDS if not (k == "ckv" and ckv_hoist))
        names = [f"dec{l}.{k}" for l in range(P.L) for k in kinds] + [f"vit{l}.{k}" for l in range(P.vL) for k in ("qkv", "fc1", "fc2")]
        if ckv_hoist:
            names.append("ckvcat")
        # the tied LM head in fp8 too (MIC_FP8_HEAD = all | bwd | 0; default all): its three GEMMs are 3.7 of the step's 8.4 TFLOP.
        # Backward: dE and dX read ONE e5m2 copy of dlogits written by the CE backward under a closed-form scale (`mic_ce_bwd_q8`; no
        # in-place gradient, no transposed copy), the e4m3 copies of E / E^T (re-made with the other weights) and the e4m3 final hidden
        # states; forward ("all"): the logits from the e4m3 operands, softmax partials as in bf16.  "bwd": forward stays bf16; "0": the
        # head as in the bf16 mode.  Needs the reduction dimensions (d, Vpad) in whole 128-byte fragments.
        mode = head if head is not None else os.environ.get("MIC_FP8_HEAD", "all")
        if mode not in ("0", "bwd", "all"):
            raise ValueError(f"MIC_FP8_HEAD / head={mode!r}: 0 | bwd | all")
        self.head = {"0": 0, "bwd": 1, "all": 2}[mode] if (P.d % 128 == 0 and P.Vpad % 128 == 0) else 0
        if self.head:
            names.append("shared")
        self.head_dy = None  # (dlogits as e5m2 [rows][Vpad] (Q8), label coefficients, labels) of the CE backward that has just run
        self.head_x = None   # the final hidden states as e4m3 (Q8) of this pass
        self.weights: Dict[str, W8] = {}
        self.w_state = torch.zeros((len(names), 2), dtype=torch.float32, device=dev)
        for i, n in enumerate(names):
            N, K = self.src(n).shape
            self.weights[n] = W8(torch.empty((N, K), dtype=E4M3, device=dev), torch.empty((K, N), dtype=E4M3, device=dev), self.w_state[i])
        self.stale = True
        self.w_part = torch.zeros((len(names), ops.fp8_amax_partials()), dtype=torch.float32, device=dev) if self.delayed else None
        self.seen = False
        self.w_async = os.environ.get("MIC_FP8_W8_ASYNC", "1") != "0"  # (A/B: 0 = weights re-quantised at the start of the next pass, on its stream)
        self.phase, self.pending = IDLE, None
        self._early, self._side = set(), None  # phase "rolled": the weights the first call took, and its stream
        segs = P.segs

        def end(n):
            sg = segs[f"dec{P.L - 1}.ckv.w" if n == "ckvcat" else "shared" if n == "shared" else n + ".w"]
            return sg.offset + sg.numel
        self._w_end = [end(n) for n in names]  # flat offset behind each weight: final once the optimizer passes up to there are issued
        self._items, self._items_key = None, None
        # one (amax, 1/scale) slot per quantised activation / gradient tensor; delayed scaling: + its table of partial maxima
        self.a_state = torch.zeros((1024, 2), dtype=torch.float32, device=dev)
        self.a_part = torch.zeros((1024, ops.fp8_amax_partials()), dtype=torch.float32, device=dev) if self.delayed else None
        self.slots: Dict[str, int] = {}
        self.ready = set()  # delayed scaling: tags whose slot carries the previous pass's amax
        self.cache: Dict = {}
        self.saved: Dict[str, Q8] = {}  # wname -> the Linear's input as quantised in the training forward (dW reads it)
        # fused emission: under delayed scaling the PRODUCER of an operand (LayerNorm, GELU / dGELU epilogue, attention backward)
        # writes the fp8 bytes itself once the tensor has a scale history (from its second pass on); MIC_FP8_FUSED=0: every operand
        # through mic_fp8_quantize again (A/B)
        self.fused = self.delayed and ln_partials and os.environ.get("MIC_FP8_FUSED", "1") != "0"

    # ------------------------------------------------------------------ weights
    def src(self, name: str):
        """the bf16 matrix behind the fp8 weight entry `name`"""
        if name == "shared":
            return self.P.w("shared")
        return self.P.ckv_cat("w")[0] if name == "ckvcat" else self.P.w(name + ".w")

    def weights_changed(self, by_optimizer: bool = False):
        self.stale = True
        if not by_optimizer:
            self.seen = False

    def _w_items(self):
        """the weight items of a delayed-scaling quantiser pass, built once (raw pointers into persistent buffers: the flat bf16
        parameter copy, the fp8 copies, the scale slots) — building them was 0.2 ms of host time in the gap between two steps"""
        key = self.P.lp.data_ptr()
        if self._items_key != key:
            self._items = [ops.fp8_item(self.src(n), w.q.shape[0], w.q.shape[1], w.state, E4M3, q=w.q, qT=w.qT, amax_next=self.w_part[i])
                           for i, (n, w) in enumerate(self.weights.items())]
            self._items_key = key
        return self._items

    def refresh_weights(self, side, upto: Optional[int] = None, wait_event=None):
        """Trainer (delayed scaling): roll the weights' amax and re-quantise them for the NEXT pass on `side` instead of in front of that
        pass.  Two calls per step: `upto` = flat offset up to which the optimizer passes have been issued (`wait_event`: recorded on
        the optimizer's stream behind them) — at the end of decoder backward: the decoder's weights go now, under the ViT's backward;
        then the final call (upto None), behind everything the current stream has enqueued, takes the rest beside the host-issued glue
        between two steps.  The first fp8 GEMM of the next pass waits for the final call's event (`wait`)."""
        if not (self.delayed and self.seen and self.w_async):
            return
        items = self._w_items()
        if upto is not None:
            todo = [i for i, e in enumerate(self._w_end) if e <= upto and i not in self._early]
            if not todo:
                return
            with torch.cuda.stream(side):
                if wait_event is not None:
                    side.wait_event(wait_event)
                with ops.pinned_stream():
                    if self.phase is not ROLLED:
                        ops.fp8_roll_amax(self.w_state, self.w_part, len(items))
                    ops.fp8_quantize([items[i] for i in todo], amax_pass=False)
            self._early.update(todo)
            self.phase, self._side = ROLLED, side
            return
        if not self.stale:
            return
        todo = [i for i in range(len(items)) if i not in self._early]
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            side.wait_event(ev)
            with ops.pinned_stream():
                if self.phase is not ROLLED:
                    ops.fp8_roll_amax(self.w_state, self.w_part, len(items))
                if todo:
                    ops.fp8_quantize([items[i] for i in todo], amax_pass=False)
            done = torch.cuda.Event()
            done.record(side)
        self.wait()  # (an event still pending here belongs to copies nobody read: waited for, not dropped)
        self.phase, self.pending, self.stale, self._early = COMPLETE, done, False, set()

    def wait(self):
        if self.phase is COMPLETE:
            torch.cuda.current_stream().wait_event(self.pending)
            self.phase, self.pending = IDLE, None

    def begin_pass(self):
        """start of a forward(+backward) pass: re-quantise the weights if they moved and no refresh has done it; current scaling:
        clear the activation slots; delayed scaling: last pass's recorded amax becomes this pass's scale source"""
        if self.phase is ROLLED:  # a step ended between the two refresh calls: its first half may still run
            torch.cuda.current_stream().wait_stream(self._side)
            self.phase, self._early = IDLE, set()
        if self.stale:
            if self.delayed and self.seen:
                ops.fp8_roll_amax(self.w_state, self.w_part, len(self.weights))
            else:
                ops.zero(self.w_state)
                if self.delayed:
                    ops.zero(self.w_part)
            self.wait()  # (a side-stream refresh of older weights may still be writing the copies)
            items = self._w_items() if self.delayed else [ops.fp8_item(self.src(n), w.q.shape[0], w.q.shape[1], w.state, E4M3, q=w.q, qT=w.qT)
                                                          for n, w in self.weights.items()]
            ops.fp8_quantize(items, amax_pass=not (self.delayed and self.seen))
            self.seen = self.delayed
            self.stale = False
        n = len(self.slots)
        if self.delayed:
            if n:
                ops.fp8_roll_amax(self.a_state, self.a_part, n)
            self.ready = set(self.slots)
        else:
            ops.zero(self.a_state[: max(n, 1)])
        self.cache = {}
        self.saved = {}
        self.head_x = None

    # ------------------------------------------------------------------ activations / gradients
    def ok(self, wname: str) -> bool:
        return wname.split(".")[-1] in self.KINDS and wname in self.weights

    def slot(self, tag: str) -> int:
        i = self.slots.get(tag)
        if i is None:
            i = self.slots[tag] = len(self.slots)
            if i >= self.a_state.shape[0]:
                raise RuntimeError("fp8: out of activation scale slots")
        return i

    def quant(self, x, rows: int, cols: int, tag: str, buf_tag: str, fmt, cache: bool = False) -> Q8:
        """bf16 x through mic_fp8_quantize (the unfused path: tensors without a scale history, operands no kernel of ours produces in
        fp8).  No transposed copy: the weight-gradient GEMM reads its operands k-major.  cache=True: x keeps its contents for the rest
        of the pass (the encoder states every layer's cross-attention projects): quantised once."""
        key = (x.data_ptr(), rows, cols, fmt)
        hit = self.cache.get(key) if cache else None
        if hit is not None:
            return hit
        # sized by the CAPACITY of x (its row count is the step-independent [B*T] / [B*S] capacity), not by this step's valid rows:
        # with packed decoder rows `rows` changes from step to step and a buffer per distinct count would never be freed
        cap = max(int(x.shape[0]), _rup(rows, self.rowpad))
        q = self.buf(buf_tag + ".q8", cap, cols, fmt)
        slot = self.slot(tag)
        st = self.a_state[slot]
        item = ops.fp8_item(x, rows, cols, st, fmt, q=q, amax_next=self.a_part[slot] if self.delayed else None)
        ops.fp8_quantize([item], amax_pass=not (self.delayed and tag in self.ready))
        out = Q8(q, st)
        if cache:
            self.cache[key] = out
        return out

    def target(self, tag: str, buf_tag: str, rows_cap: int, cols: int, fmt) -> Optional[Q8Target]:
        """the tensor `tag` as its producer is to EMIT it: fused emission on (delayed scaling) and a scale history for this tensor
        (second pass on); else None: the producer writes bf16 and `quant` follows."""
        if not (self.fused and tag in self.ready):
            return None
        slot = self.slot(tag)
        st, part = self.a_state[slot], self.a_part[slot]
        q = self.buf(buf_tag + ".q8", rows_cap, cols, fmt)
        return Q8Target(q, st, ops.fp8_out(q, st, part), (st, part))

    @staticmethod
    def dy_buf(wname: str, par: int) -> str:
        """buffer of the e5m2 gradient w.r.t. the OUTPUT of the fp8 Linear `wname`; `par`: layer parity (the deferred weight-gradient
        launch of a layer reads it while the next layer's backward already writes the other buffer)"""
        return f"f8.{wname.split('.')[0].rstrip('0123456789')}.{wname.split('.')[-1]}.dy.{par}"

    def dy_target(self, wname: str, par: int, cap: int) -> Optional[Q8Target]:
        """fused-emission target (see `target`) for that gradient — the dy the backward GEMMs of `wname` read"""
        return self.target(wname + ".dy", self.dy_buf(wname, par), cap, self.P.w(wname + ".w").shape[0], E5M2)
