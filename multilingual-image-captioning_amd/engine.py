"""Kernel sequencing for the captioning hot path: ViT encoder -> projection -> mBART decoder -> tied head, forward
(+loss) and the hand-derived backward.  Pure orchestration: every tensor op is a libmic_hip.so kernel (ops.*);
torch supplies device memory and the current HIP stream only.

Module graph restated from `modeling_clip_vision_mbart.py:67-115, 146-192` (composition) and SURVEY Appendix B
(third-party block structure).  Activations live in row-padded [rows_pad][width] buffers (rows_pad = multiple of 128,
pad rows stay zero) so weight-gradient GEMMs can reduce over the padded row count.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, Optional

import torch

from . import _lib as L
from . import ops
from .fp8_state import E4M3, E5M2, Q8, Fp8State, Fp8Views
from .params import ParamStore, _rup

ROWPAD = 128


def _mix(seed: int, site: int) -> int:
    x = (seed * 0x9E3779B1 + site * 0x85EBCA6B + 0x27D4EB2F) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x ^= x >> 12
    return x & 0xFFFFFFFF


def packed_attn_tiled(Tq_max: int, Tk: int) -> bool:
    """which packed attention cores one call takes: the one-tile kernels while queries and keys fit one 64x64 tile, the tiled ones
    (`ops.attn_*_packed_tiled`) beyond.  Self-attention asks with (T, T), cross-attention with (T, S): at T <= 64 < S only the
    cross-attention leaves the one-tile kernels.
    This is the engine's one-tile rule for packed and dense rows alike: `Engine.attn_forward` / `attn_backward` choose by it, and fp8
    emission out of the attention backward (`dy8_target` of its q/k/v projections) is asked for only where it answers False."""
    return Tq_max > 64 or Tk > 64


class Shortlist:
    """A vocabulary shortlist for the LM head (generate(allowed_token_ids=...)): the Ns sorted unique token ids `map`, the rows
    `E` [Ns_pad][d] of the tied embedding they name (compute dtype) and their entries `bias` [Ns_pad] of final_logits_bias (fp32);
    Ns_pad = Ns rounded up to 128, the padding rows and entries zero.  The tensors are allocated once and stay where they are — captured
    decoder steps hold their addresses — and `refresh()` re-gathers them in place when the weights have moved (ParamStore.version: the
    rule Engine.ln_folded follows)."""

    def __init__(self, engine: "Engine", ids, key):
        P = engine.P
        self.engine, self.key = engine, key            # key = (Ns, digest of the ids): the identity decode plans are keyed by
        self.ids = ids                                 # numpy int32, sorted unique (host copy: token -> column lookups)
        self.Ns, self.Ns_pad = int(ids.size), _rup(int(ids.size), ROWPAD)
        self.map = torch.from_numpy(ids).to(P.device)
        self._rows = self.map.long()                   # (index_select wants int64)
        self.E = torch.zeros((self.Ns_pad, P.d), dtype=P.dtype, device=P.device)
        self.bias = torch.zeros(self.Ns_pad, dtype=torch.float32, device=P.device)
        self.version = None

    def column(self, token: int) -> int:
        """the column of vocabulary id `token` (which must be on the list)"""
        import numpy as np

        i = int(np.searchsorted(self.ids, token))
        if i >= self.Ns or int(self.ids[i]) != int(token):
            raise ValueError(f"token {token} is not in the vocabulary shortlist")
        return i

    def refresh(self):
        P = self.engine.P
        ver = getattr(P, "version", 0)
        if ver != self.version:
            ops.copy_rows(P.w("shared"), self.E, self.Ns, P.d, src_idx=self.map)
            torch.index_select(P.f32("flb"), 0, self._rows, out=self.bias[: self.Ns])
            self.version = ver


class Engine(Fp8Views):
    def __init__(self, store: ParamStore):
        self.P = store
        self.dt = store.dtype
        self.dev = store.device
        self._bufs: Dict[str, torch.Tensor] = {}
        mc = store.cfg.mbart_config
        self.gelu = L.ACT_IDS[getattr(mc, "gelu_variant", "tanh")]
        self.dec_eps = float(getattr(mc, "decoder_ln_eps", 1e-6))
        self.vit_eps = float(store.cfg.clip_vision_config.layer_norm_eps)
        self.p_drop = float(mc.dropout)
        self.embed_scale = math.sqrt(store.d) if mc.scale_embedding else 1.0
        self.defer_embed = False  # True: leave the sparse tied-embedding rows (ids, dh0) to the caller (data parallel)
        self.embed_rows = None     # (ids, dh0 buffer, M) of the last backward when deferred
        self._dw_queue = []
        self._cs_queue = []
        self._dw8_queue = []     # (fp8 projections: their weight-gradient GEMMs ...
        self._cs8_queue = []     # ... and bias gradients: column sums over the e5m2 bytes of dy)
        self.on_free = []  # callables run by free_buffers() before the buffers go (decode plans drop their captured graphs)
        self.fp8 = False
        self.f8: Optional[Fp8State] = None  # the fp8 operands' state while the projections run as fp8 GEMMs (set_gemm_dtype)
        self.use_head_stats = os.environ.get("MIC_HEAD_STATS", "1") != "0"  # softmax partials out of the LM-head GEMM (A/B switch)
        self.grad_progress = None  # callable(offset): every gradient with flat offset < offset is final (DDP overlap)
        self.on_embed_rows = None  # callable(): single process, right behind the input-embedding scatter at the end of decoder backward
        # set by Trainer(param_groups=...) for a step in which every segment of the image tower is frozen: loss_and_grads stops at the
        # bridge (vit_backward_bridge); the gradients of the ViT segments are then NOT computed — their part of ParamStore.grad keeps
        # whatever it held (the atomic region: the step's zeros)
        self.skip_vit_backward = False
        # weight-gradient GEMMs on a second stream (bf16 / f32 GEMM modes): nothing but the optimizer depends on dW, so a layer's
        # grouped dW launch runs beside the NEXT layer's dX chain (LayerNorm / attention backward and the small dX GEMMs leave
        # most CUs idle).  The gradient operands dW reads are double-buffered by layer parity; A/B switch MIC_DW_OVERLAP=0|1.
        self.dw_overlap = self.dev.type == "cuda" and os.environ.get("MIC_DW_OVERLAP", "1") != "0"
        # decoder-step LayerNorms folded around the GEMMs (bfloat16 generate path): A/B switch
        self.decode_ln_fold = self.dev.type == "cuda" and os.environ.get("MIC_DECODE_LNFOLD", "1") != "0"
        self._ckv_hoist = os.environ.get("MIC_CKV_HOIST", "1") != "0"
        # several captions per image (kv_group > 1), one-tile sizes: the shared-K/V kernels, or MIC_ATTN_SHARED=tiled: an image's
        # captions as one sequence of the existing cores (A/B; beyond one tile that is the only form)
        self.attn_shared_tiled = os.environ.get("MIC_ATTN_SHARED", "") == "tiled"
        self._lnf = {}
        self._lnf_version = -1
        self._dw_stream = None
        # LM-head backward as NT launches of the four-wave kernel (k-contiguous copies: dlogits^T from the CE backward, h^T, E^T);
        # MIC_HEAD_NT=0: the k-major launches of rounds 1-4 (A/B)
        self.head_nt = os.environ.get("MIC_HEAD_NT", "1") != "0"
        # LayerNorm backward: gamma / beta gradients as per-block partial sums reduced later with the layer's weight-gradient launches
        # (no atomics on the critical path, a fixed summation order); MIC_LN_PARTIALS=0: fp32 atomics inside the kernel (A/B)
        self.ln_partials = os.environ.get("MIC_LN_PARTIALS", "1") != "0"
        self._lnp_queue = []
        self._head_nt_state = None   # (dlogits^T, Kp) of the CE backward that has just run
        self.fp8_head = 0            # fp8 GEMM mode: the tied head's GEMMs on fp8 operands too (set_gemm_dtype)
        self._ET_version, self._ET_event = -1, None
        self._dw_events = []
        # weight-gradient launches behind every n-th layer: 2 in fp8 mode (its two GEMM streams alternate rather than overlap — half as
        # many hand-overs: 14.87 -> 14.75 ms), 1 in bf16 (2 measured level); MIC_DW_EVERY=<n> forces a value (A/B)
        self.dw_every = int(os.environ.get("MIC_DW_EVERY", "0"))
        self.dw_late_flush = os.environ.get("MIC_DW_LATE_FLUSH", "1") != "0"  # see dw_fence (A/B: 0 = the weight-gradient launch in front of that LayerNorm backward)
        self._dw_side = False  # True while launching on the dW stream
        self._ckv_block_name = None  # set while the all-layer cross k/v weight gradient (one launch) sits in the dW queue

    # ------------------------------------------------------------------ fp8 GEMM operands (BASELINE configs[4])
    def set_gemm_dtype(self, name, scaling: str = "delayed", head: Optional[str] = None):
        """"fp8": the QKV / FFN projections run as OCP fp8 GEMMs — e4m3 activations and weights, e5m2 gradients, one scale per
        tensor, fp32 accumulate (forward, dX and dW).  None / "bf16": the storage dtype.
        scaling="current": every activation / gradient tensor is scaled by its own absolute maximum (two passes over the
        tensor: amax, then quantise).  scaling="delayed" (default; the usual production recipe): the scale comes from the
        amax the same tensor had in the previous pass, the quantiser records the new amax on the way (one pass); values
        that outgrow the old amax saturate at +-FMAX for that one pass.  A tensor seen for the first time is scaled by its
        current amax.  Weights are re-quantised once per optimizer step — with their current amax ("current"), or ("delayed")
        with the amax of the previous step's weights, recorded by the previous quantiser pass: an optimizer step moves a weight
        by ~lr, so the one-step-old maximum is the current one to fp8 precision and the amax pass over 246 M parameters goes;
        weights that arrive any other way (params setter, checkpoint restore) start again from their current amax.
        Under delayed scaling a tensor WITH a scale history is not quantised by a launch of its own: its producer (LayerNorm forward /
        backward, the GELU / dGELU epilogue of the fp8 GEMM, attention backward) writes the fp8 bytes (`Fp8State.target`, `fp8_fused`);
        the weight copies of the next pass are made on a side stream behind the optimizer (`Fp8State.refresh_weights`).
        head = "all" | "bwd" | "0" (default: MIC_FP8_HEAD, else "all"): the tied LM head's three GEMMs / its two backward GEMMs / none
        of them on fp8 operands (see fp8_state.py).  The operands' state lives in `self.f8` (None outside the fp8 mode)."""
        if name in (None, "bf16", "bfloat16", "f32", "float32"):
            self.fp8, self.f8 = False, None
            return
        if name != "fp8":
            raise ValueError(f"unknown gemm_dtype {name!r}")
        if scaling not in ("delayed", "current"):
            raise ValueError(f"fp8 scaling must be 'delayed' or 'current', got {scaling!r}")
        if self.dt != torch.bfloat16:
            raise ValueError("gemm_dtype='fp8' needs the bfloat16 storage mode (dtype=bfloat16)")
        self.f8 = Fp8State(self.P, self.buf, ROWPAD, scaling, head, self._ckv_hoist, self.ln_partials)
        self.fp8, self.fp8_scaling, self.fp8_head = True, scaling, self.f8.head

    def storage_dtype_gemms(self):
        """context: every Linear runs in the storage dtype (bf16) even when the trainer switched the projections to fp8 — the
        inference entry points (`encode`, `decode`, `generate`) are not part of a train / eval pass: nothing re-quantises the
        weights for them or rolls the activation scales, so fp8 launches there would read stale (or never written) copies"""
        @contextlib.contextmanager
        def ctx():
            keep = self.fp8
            self.fp8 = False
            try:
                yield
            finally:
                self.fp8 = keep
        return ctx()

    def _fp8_begin_pass(self):
        if self.fp8:
            self.f8.begin_pass()

    def _fp8_ok(self, wname: str) -> bool:
        return self.fp8 and self.f8.ok(wname)

    def dy8_target(self, wname: str, par: int, cap: int):
        """`Fp8State.dy_target` when the Linear `wname` runs in fp8, else None"""
        return self.f8.dy_target(wname, par, cap) if self._fp8_ok(wname) else None

    def ln_q8(self, x, ln: str, eps: float, a_name: str, cap: int, mean, rstd, rows: int, wname: str, q_tag: str, **kw):
        """LayerNorm `ln` of x whose output feeds Linear `wname`: (a bf16 or None, x8 = Q8 or None).  Fused fp8 emission when
        that Linear runs in fp8 and its input has a scale history: the normalised rows leave as e4m3 bytes only."""
        P = self.P
        width = x.shape[-1]
        t = self.f8.target(wname + ".x", q_tag + wname.split(".")[-1] + ".x", cap, width, E4M3) if self._fp8_ok(wname) else None
        if t is not None:
            ops.layernorm_fwd(x, P.f32(ln + ".g"), P.f32(ln + ".b"), eps, None, mean, rstd, rows=rows, q8=t.out, **kw)
            return None, t.q8
        a = self.buf(a_name, cap, width)
        ops.layernorm_fwd(x, P.f32(ln + ".g"), P.f32(ln + ".b"), eps, a, mean, rstd, rows=rows, **kw)
        return a, None

    def _done(self, seg_name: str):
        """Report that the gradient segment `seg_name` (and, by layout order, everything before it) is final."""
        if self.grad_progress is not None:
            if self._dw_events and not self._dw_side:
                torch.cuda.current_stream().wait_event(self._dw_events[-1])  # "everything before it" includes the dW stream's work
            s = self.P.segs[seg_name]
            self.grad_progress(s.offset + s.numel)

    # ------------------------------------------------------------------ buffers
    def buf(self, name: str, rows: int, cols: int, dtype=None) -> torch.Tensor:
        """The buffer `name` of capacity `rows` x `cols`: zeros on first touch, the SAME tensor (whatever the last call left in it) ever
        after.  The buffer contract (table and tests: tests/util_poison.py, tests/test_poison_gpu.py):
        SCRATCH — rows [0, rows): a caller writes what it reads, in every call, and bounds its reads by the call's valid rows; nothing
          may depend on the previous contents.  That is every buffer handed out here and by `vec` except the STATE ones below; the
          decoder step's `g.ehs` / `g.ckv<l>` are the sequence's state between the steps of one `decode()` sequence.
        REST — rows [rows, allocation) (the padding to 128 rows): zero for ever, no kernel may write them — the fp32 weight-gradient
          GEMMs and the patch-embedding dW reduce over the padded row count.  (Elsewhere: unused `Fp8State` slots and a shortlist's
          padding are zero; the workspace of mic_embed_rows_add_det is owner = INT_MAX, count = 0, last = -1, multi_count = 0.)
        STATE — `w.sharedT` (E^T, a derived weight copy: `shared_T`) and `ones_i32` (built once, only grows).  (Elsewhere: weights,
          AdamW moments, `acc`, the Trainer's `hyper`, the fp8 scale history and weight copies, LayerNorm folds, shortlists, a decode
          plan's constants.)"""
        dtype = dtype or self.dt
        key = (name, rows, cols, dtype)  # (a tuple: this lookup runs ~1500 times per train step on the host)
        t = self._bufs.get(key)
        if t is None:
            t = torch.zeros((_rup(max(rows, 1), ROWPAD), cols), dtype=dtype, device=self.dev)
            self._bufs[key] = t
        return t

    def vec(self, name: str, n: int, dtype=torch.float32) -> torch.Tensor:
        key = (name, n, dtype)
        t = self._bufs.get(key)
        if t is None:
            t = torch.zeros(n, dtype=dtype, device=self.dev)
            self._bufs[key] = t
        return t

    def free_buffers(self):
        """drop every scratch / activation buffer.  Captured decoder-step graphs hold raw pointers into these buffers (and into
        the LayerNorm-folded weights): whoever captured them registered a callback in `on_free` and is told first."""
        for cb in list(self.on_free):
            cb()
        self._bufs.clear()
        self._ET_version, self._ET_event, self._head_nt_state = -1, None, None
        self._lnf = {}
        self._lnf_version = -1

    # ------------------------------------------------------------------ attention cores: which entry point takes a call
    def attn_forward(self, q, k, v, out, lse, B, H, Tq, Tk, *, ldq, ldk, ldv, ldo, pack=None, kv_packed=False, key_mask=None, causal=False,
                     kv_group=1):
        """out, lse = attention of q over k / v.  pack = (q_off, q_len, rows) or None: packed query rows take the packed cores (one-tile
        or tiled by `packed_attn_tiled`), which know no key mask — every position of a packed sequence is valid; kv_packed: the keys
        are those packed rows too (self-attention), not [B][Tk] rows (cross-attention).
        kv_group = G > 1 (cross-attention only: no mask, not causal, not kv_packed): the B = n_img * G query sequences are image-major
        and sequence b attends the Tk rows of image b // G.  One tile: the shared-K/V kernels.  Beyond one tile (or MIC_ATTN_SHARED=tiled)
        an image's G consecutive captions are ONE sequence of the existing cores — cross-attention couples no two queries — dense rows
        as B' = n_img, Tq' = G*Tq, packed rows through the grouped description pack[3:5] (`train.group_packed_rows`)."""
        if kv_group > 1:
            n_img, G = self._kv_group_call(B, kv_group, kv_packed, key_mask, causal)
            if not (packed_attn_tiled(Tq, Tk) or self.attn_shared_tiled):
                q_off, q_len = (None, None) if pack is None else pack[:2]
                ops.attn_fwd_shared(q, k, v, out, n_img, G, H, Tq, Tk, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, q_off=q_off, q_len=q_len, lse=lse)
            elif pack is None:
                ops.attn_fwd(q, k, v, out, n_img, H, G * Tq, Tk, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, lse=lse)
            else:
                ops.attn_fwd_packed_tiled(q, k, v, out, n_img, H, G * Tq, Tk, pack[3], pack[4], kv_packed=False, ldq=ldq, ldk=ldk, ldv=ldv,
                                          ldo=ldo, lse=lse)
        elif pack is None:
            ops.attn_fwd(q, k, v, out, B, H, Tq, Tk, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, key_mask=key_mask, causal=causal, lse=lse)
        else:
            fwd = ops.attn_fwd_packed_tiled if packed_attn_tiled(Tq, Tk) else ops.attn_fwd_packed
            fwd(q, k, v, out, B, H, Tq, Tk, pack[0], pack[1], kv_packed=kv_packed, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, causal=causal, lse=lse)

    def _kv_group_call(self, B, G, kv_packed, key_mask, causal):
        if kv_packed or key_mask is not None or causal or B % G:
            raise ValueError(f"attention with shared keys / values (kv_group={G}): cross-attention only (no key mask, not causal, keys not the "
                             f"packed rows) on a whole number of images (B={B})")
        return B // G, G

    def attn_backward(self, q, k, v, out, dout, lse, B, H, Tq, Tk, *, ldq, ldk, ldv, ldo, lddo, grads=None, ldg=None, grads8=None, pack=None,
                      kv_packed=False, key_mask=None, causal=False, kv_group=1):
        """the backward of `attn_forward` (same pack / kv_packed / key_mask / causal / kv_group).  Either grads = (dq, dk, dv) with their
        row strides ldg, or grads8 = (dQ's `fp8_out`, dK's `fp8_out`, dV's fp8 view): the gradients leave as fp8 bytes, one 64x64 tile
        only.  kv_group = G > 1: dk / dv [n_img * Tk rows] are the sums over an image's G captions (no fp8 emission)."""
        q_off, q_len = (None, None) if pack is None else pack[:2]
        if kv_group > 1:
            n_img, G = self._kv_group_call(B, kv_group, kv_packed, key_mask, causal)
            if grads8 is not None:
                raise ValueError("attention backward with shared keys / values: no fp8 emission of dK / dV")
            ld = dict(ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, lddo=lddo, lddq=ldg[0], lddk=ldg[1], lddv=ldg[2])
            if not (packed_attn_tiled(Tq, Tk) or self.attn_shared_tiled):
                ops.attn_bwd_shared(q, k, v, out, dout, lse, *grads, n_img, G, H, Tq, Tk, q_off=q_off, q_len=q_len, **ld)
            elif pack is None:
                ops.attn_bwd(q, k, v, out, dout, lse, *grads, n_img, H, G * Tq, Tk, **ld)
            else:
                ops.attn_bwd_packed_tiled(q, k, v, out, dout, lse, *grads, n_img, H, G * Tq, Tk, pack[3], pack[4], kv_packed=False, **ld)
            return
        if grads8 is not None:
            if packed_attn_tiled(Tq, Tk):
                raise ValueError(f"attention backward: fp8 emission needs one 64x64 tile per sequence (Tq={Tq} Tk={Tk})")
            ops.attn_bwd_q8(q, k, v, out, dout, lse, *grads8, B, H, Tq, Tk, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, lddo=lddo, q_off=q_off, q_len=q_len,
                            kv_packed=kv_packed and pack is not None, key_mask=key_mask if pack is None else None, causal=causal)
            return
        ld = dict(ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, lddo=lddo, lddq=ldg[0], lddk=ldg[1], lddv=ldg[2])
        if pack is None:
            ops.attn_bwd(q, k, v, out, dout, lse, *grads, B, H, Tq, Tk, key_mask=key_mask, causal=causal, **ld)
        else:
            bwd = ops.attn_bwd_packed_tiled if packed_attn_tiled(Tq, Tk) else ops.attn_bwd_packed
            bwd(q, k, v, out, dout, lse, *grads, B, H, Tq, Tk, q_off, q_len, kv_packed=kv_packed, causal=causal, **ld)

    # ------------------------------------------------------------------ small helpers
    def linear(self, x, wname, out, M, *, act=0, zout=None, residual=None, drop_seed=None, bias=True, save_tag=None, fp8=True,
               stable_input=False, x8=None, out8=None):
        """save_tag (fp8 mode, training forward): the fp8 copy of x is kept under that name for the weight-gradient GEMM of backward
        (dW = dy^T x reads dy and x k-major, as they lie).  x8 (a Q8): x already exists as fp8 bytes (fused emission by its
        producer; `x` may be None).  out8 (a Q8Target): the result leaves as fp8 bytes (the GELU output of FFN-in, whose only
        reader is the fp8 FFN-out projection); returns its Q8 then."""
        P = self.P
        w = P.w(wname + ".w")
        N, K = w.shape
        p = self.p_drop if drop_seed is not None else 0.0
        if fp8 and self._fp8_ok(wname):
            f8 = self.f8
            f8.wait()
            w8 = f8.weights[wname]
            if x8 is None:
                x8 = f8.quant(x, M, K, wname + ".x", (save_tag or "f8.") + wname.split(".")[-1] + ".x", E4M3, cache=stable_input)
            if save_tag is not None:
                f8.saved[wname] = x8
            kw = dict(bias=P.f32(wname + ".b") if bias else None, act=act, zout=zout, residual=residual, dropout_p=p, dropout_seed=drop_seed or 0,
                      a_scale_inv=x8.scale_inv, b_scale_inv=w8.scale_inv)
            if out8 is not None:
                ops.gemm(x8.q, w8.q, out8.q, M, N, K, c_q8=out8.c_q8, **kw)
                return out8.q8
            return ops.gemm(x8.q, w8.q, out, M, N, K, **kw)
        return ops.gemm(x, w, out, M, N, K, bias=P.f32(wname + ".b") if bias else None, act=act, zout=zout,
                        residual=residual, dropout_p=p, dropout_seed=drop_seed or 0)

    def linear_bwd(self, wname, x, dy, M, *, dx=None, zin=None, dact=0, dx_accumulate=False, bias=True, defer=False, x_tag=True,
                   dy8=None, dx8=None, par=0):
        """dW = dy^T x (fp32, overwrite), db = colsum(dy), optionally dx = (dy W) [* act'(zin)].
        defer=True queues the weight-gradient GEMM (nothing but the optimizer depends on it): the caller keeps dy and x
        intact until flush_dw() launches the layer's queue as ONE grouped GEMM (36..256-tile problems fill the chip
        only together).  fp8 projections: dy8 (a Q8) when dy's producer emitted the e5m2 bytes itself (`dy` may be None),
        dx8 (a Q8Target) when dx is to leave as fp8 bytes (the dGELU-scaled dX of FFN-out = the dy of FFN-in); par = layer
        parity of the buffer an unfused dy is quantised into (it is read by the deferred launches of its layer)."""
        P = self.P
        w = P.w(wname + ".w")
        N, K = w.shape
        Mp = _rup(M, ROWPAD)
        if self._fp8_ok(wname) and x_tag is not None:
            # fp8: dy as e5m2 bytes [M][N] — row-major for dX = dy W (NT against W^T, quantised once per step), k-major for
            # dW = dy^T x (TN: both operands as their producers wrote them); x as saved by the forward pass
            f8 = self.f8
            if dy8 is None:
                dy8 = f8.quant(dy, M, N, wname + ".dy", f8.dy_buf(wname, par), E5M2)
            x8 = f8.saved.get(wname)
            if x8 is None:
                raise RuntimeError(f"fp8 backward of {wname}: the forward pass did not keep the fp8 copy of its input (save_tag missing)")
            w8 = f8.weights[wname]
            ga = ops.gemm_args(dy8.q, x8.q, P.g(wname + ".w"), N, K, Mp, a_kmajor=True, b_kmajor=True, k_valid=M,
                               a_scale_inv=dy8.scale_inv, b_scale_inv=x8.scale_inv)
            cs = (dy8.q, P.g(wname + ".b"), dy8.scale_inv, M, N) if bias else None  # (into the pre-zeroed atomic region)
            if defer:
                self._dw8_queue.append((ga, wname, bias))
                if cs is not None:
                    self._cs8_queue.append(cs)
            else:
                ops.gemm_grouped([ga])
                if cs is not None:
                    ops.colsum_q8_grouped([cs])
            if dx8 is not None:
                ops.gemm(dy8.q, w8.qT, dx8.q, M, K, N, zin=zin, dact=dact, a_scale_inv=dy8.scale_inv, b_scale_inv=w8.scale_inv, c_q8=dx8.c_q8)
            elif dx is not None:
                ops.gemm(dy8.q, w8.qT, dx, M, K, N, zin=zin, dact=dact, accumulate=dx_accumulate, a_scale_inv=dy8.scale_inv, b_scale_inv=w8.scale_inv)
            if not defer:
                self._done(wname + ".w")
            return dx
        # bf16: the bias gradient colsum(dy) rides on the dW GEMM (row sums of its A operand dy^T, from the fragments the
        # kernel already holds; fp32 atomics into the pre-zeroed atomic region).  fp32 mode keeps the separate column sum.
        fuse = bias and self.dt == torch.bfloat16
        rs = dict(a_rowsum=P.g(wname + ".b"), rowsum_k=M) if fuse else {}
        if self.dt == torch.bfloat16:
            rs["k_valid"] = M  # reduction rows behind the M valid ones count as zero (packed batches: M changes from step to step)
        if defer:
            self._dw_queue.append((ops.gemm_args(dy, x, P.g(wname + ".w"), N, K, Mp, a_kmajor=True, b_kmajor=True, **rs), wname, bias))
        else:
            ops.gemm(dy, x, P.g(wname + ".w"), N, K, Mp, a_kmajor=True, b_kmajor=True, **rs)
        if bias and not fuse:
            if defer:
                self._cs_queue.append((dy, P.g(wname + ".b"), M, N, dy.stride(0)))
            else:
                ops.colsum(dy, P.g(wname + ".b"), M, N, dy.stride(0), accumulate=True)  # region pre-zeroed once per step
        if dx is not None:
            ops.gemm(dy, w, dx, M, K, N, b_kmajor=True, zin=zin, dact=dact, accumulate=dx_accumulate)
        if not defer:
            self._done(wname + ".w")
        return dx

    def ln_folded(self, wname: str, ln: str):
        """(gamma o W, colsum, bias') of Linear `wname` behind LayerNorm `ln` (mic_ln_fold_weight), rebuilt when the weights
        changed (ParamStore.version): the operands of a LayerNorm-folded GEMM (mic_gemm_args.a_ln_stats)"""
        P = self.P
        ver = getattr(P, "version", 0)
        if ver != self._lnf_version:
            self._lnf_fresh = set()
            self._lnf_version = ver
        hit = self._lnf.get(wname)
        if hit is None:
            w = P.w(wname + ".w")
            hit = self._lnf[wname] = (torch.empty_like(w), torch.empty(w.shape[0], dtype=torch.float32, device=self.dev),
                                      torch.empty(w.shape[0], dtype=torch.float32, device=self.dev))
        if wname not in self._lnf_fresh:
            ops.ln_fold_weight(P.w(wname + ".w"), P.f32(ln + ".g"), P.f32(ln + ".b"), P.f32(wname + ".b"), *hit)
            self._lnf_fresh.add(wname)
        return hit

    def dyb(self, name: str, l: int, rows: int, cols: int) -> torch.Tensor:
        """gradient buffer that a queued weight-gradient GEMM reads: one per layer parity when dW runs on its own stream (the
        next layer's backward rewrites the other one), a single buffer otherwise"""
        return self.buf(f"{name}.{self._par(l)}" if self._dw_on() else name, rows, cols)

    def ln_bwd(self, tag: str, l: int, x, ln: str, mean, rstd, dy, dx, rows: int, **kw):
        """LayerNorm backward of the LayerNorm named `ln` (parameters ln + ".g" / ".b"): dx (and the kwargs' by-products) now, the
        gamma / beta gradients either by atomics inside the kernel or — default — as block partials in a per-(call site, layer
        parity) buffer, summed by the next flush_dw() (the buffer discipline of dyb())"""
        P = self.P
        if not self.ln_partials:
            return ops.layernorm_bwd(x, P.f32(ln + ".g"), mean, rstd, dy, dx, P.g(ln + ".g"), P.g(ln + ".b"), rows=rows, **kw)
        width = x.shape[-1]
        part = self.buf(f"lnp.{tag}.{self._par(l)}", 2 * ops.layernorm_bwd_blocks(1 << 30), width, torch.float32)  # [2][blocks <= cap][width]
        ops.layernorm_bwd_partials(x, P.f32(ln + ".g"), mean, rstd, dy, dx, part, rows=rows, **kw)  # (kw may carry q8 / q8_of_dx: fused fp8 emission)
        self._lnp_queue.append((part, ops.layernorm_bwd_blocks(rows), width, P.g(ln + ".g"), P.g(ln + ".b"), False))
        return dx

    def _dw_on(self) -> bool:
        return self.dw_overlap

    def _par(self, l: int) -> int:
        """index of layer l's copy of a gradient buffer that a queued weight-gradient launch reads: 2 x dw_every copies in turn"""
        return l % (2 * self._dw_every_now())

    def _dw_every_now(self) -> int:
        if not self._dw_on():
            return 1  # no second stream: single buffers, the launches go out in front of every layer's last LayerNorm backward
        return self.dw_every if self.dw_every > 0 else (2 if self.fp8 else 1)

    def _dw_flush_layer(self, l: int) -> bool:
        """weight-gradient launches go out behind every `dw_every`-th layer (and behind layer 0): with 2 x dw_every buffer copies the
        launch that read a copy is the one before the latest when that copy is rewritten, exactly as with one launch per layer"""
        return l % self._dw_every_now() == 0

    def dw_fence(self) -> bool:
        """The wait half of flush_dw(), issued on its own IN FRONT of the layer's last LayerNorm backward: the step's stream waits
        for the most recent weight-gradient launch (the one that read the parity buffers that LayerNorm backward and the next layer
        rewrite); the launch half follows behind that kernel (`flush_dw(fence=False)`), so the critical chain's kernel is in its
        queue before the weight-gradient group is released onto the chip.  False: no second stream — flush_dw() has to come first."""
        if not (self._dw_on() and self.dw_late_flush):
            return False
        if self._dw_events:
            torch.cuda.current_stream().wait_event(self._dw_events[-1])
        return True

    def flush_dw(self, fence: bool = True):
        """Launch the layer's queued weight-gradient GEMMs (and bias column sums) as grouped launches — on the dW stream when
        enabled: it waits for everything enqueued so far (the operands' producers), main goes on with the next layer and
        only waits for the dW launch of TWO layers back (the one that read the buffers the next layer is about to rewrite;
        fence=False: dw_fence() has issued that wait already)."""
        if not (self._cs_queue or self._dw_queue or self._lnp_queue or (self.fp8 and (self._dw8_queue or self._cs8_queue))):
            return
        side = None
        if self._dw_on():
            if self._dw_stream is None:
                n = int(os.environ.get("MIC_DW_CUS", "0"))  # A/B: the weight-gradient stream on the LAST n CUs of the mask only
                self._dw_stream = ops.cu_masked_stream(256 - n, n, self.dev) if n > 0 else ops.role_stream(self.dev, "dw")
            side = self._dw_stream
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            side.wait_event(ev)
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            with (ops.pinned_stream() if side is not None else contextlib.nullcontext()):
                self._dw_side = side is not None
                try:
                    self._flush_dw_launches()
                finally:
                    self._dw_side = False
            if side is not None:
                done = torch.cuda.Event()
                done.record(side)
                self._dw_events.append(done)
        if side is not None and len(self._dw_events) >= 2:
            if fence:
                torch.cuda.current_stream().wait_event(self._dw_events[-2])
            del self._dw_events[:-2]

    def dw_join(self):
        """end of backward: the step's stream waits for the dW stream (next forward rewrites the saved activations dW reads)"""
        if self._lnp_queue:
            self.flush_dw()  # LayerNorm parameter gradients queued behind the last layer's flush
        if self._dw_events:
            torch.cuda.current_stream().wait_event(self._dw_events[-1])
            self._dw_events = []

    def _flush_dw_launches(self):
        if self._lnp_queue:
            ops.ln_param_grads(self._lnp_queue)
            self._lnp_queue = []
        if self._cs_queue:
            ops.colsum_grouped(self._cs_queue)
            self._cs_queue = []
        names = []
        if self.fp8 and self._cs8_queue:
            ops.colsum_q8_grouped(self._cs8_queue)
            self._cs8_queue = []
        if self.fp8 and self._dw8_queue:
            ops.gemm_grouped([q[0] for q in self._dw8_queue])
            names += [q[1] for q in self._dw8_queue]
            self._dw8_queue = []
        if self._dw_queue:
            ops.gemm_grouped([q[0] for q in self._dw_queue])
            names += [q[1] for q in self._dw_queue]
            self._dw_queue = []
        # every queued gradient of the layer is in flight on this stream: report the one that sits last in the flat layout.  The
        # cross-attention k/v weights of ALL layers form one block behind decoder layer 0 (ParamStore.ckv_cat): a per-layer k/v
        # gradient (fp8 GEMMs / MIC_CKV_HOIST=0) must not count here — its offset lies behind every decoder layer, reporting it at
        # layer L-1 would declare the gradients of layers L-2 .. 0 final before their GEMMs have run.  The hoisted launch queues the
        # whole block under the name of its LAST member at the end of decoder backward; the per-layer path reports the block once,
        # after layer 0 (decoder_backward).
        names = [n for n in names if not n.endswith(".ckv") or n == self._ckv_block_name]
        if names:
            self._done(max(names, key=lambda n: self.P.segs[n + ".w"].offset) + ".w")

    # ------------------------------------------------------------------ ViT
    def vit_forward(self, pixels: torch.Tensor, save: bool, trunc_int32: bool = False):
        """pixels [B,img,img,3] fp32 NHWC -> (last hidden [B*S,vd] NOT post-layernormed, ehs [B*S,d])."""
        P = self.P
        B = pixels.shape[0]
        S, vd, vf, H = P.S, P.vd, P.vffn, P.vH
        Mv, Mp = B * S, B * (S - 1)
        pk = P.ps * P.ps * 3
        patches = self.buf("v.patches", Mp, pk)
        ops.im2col(pixels, patches, B, P.img, P.ps, pk, trunc_int32)
        pe = self.buf("v.pe", Mp, vd)
        ops.gemm(patches, P.w("patch.w"), pe, Mp, vd, pk)
        emb = self.buf("v.emb", Mv, vd)
        ops.vit_assemble(pe, P.f32("vit.cls"), P.f32("vit.pos"), emb, B, S, vd, vd)
        x = self.buf("v.x0", Mv, vd)
        st = self.buf("v.pre.stats", 2, _rup(Mv, ROWPAD), torch.float32)
        ops.layernorm_fwd(emb, P.f32("vit.pre_ln.g"), P.f32("vit.pre_ln.b"), self.vit_eps, x, st[0], st[1], rows=Mv)
        for l in range(P.vL):
            tag = f"v{l}." if save else "v_."
            p = f"vit{l}."
            st1 = self.buf(tag + "st1", 2, _rup(Mv, ROWPAD), torch.float32)
            a1, a1_8 = self.ln_q8(x, p + "ln1", self.vit_eps, tag + "a1", Mv, st1[0], st1[1], Mv, p + "qkv", tag)
            qkv = self.buf(tag + "qkv", Mv, 3 * vd)
            self.linear(a1, p + "qkv", qkv, Mv, save_tag=tag if save else None, x8=a1_8)
            ctx = self.buf(tag + "ctx", Mv, vd)
            lse = self.vec(tag + "lse", B * H * S)
            self.attn_forward(qkv, qkv[:, vd:], qkv[:, 2 * vd:], ctx, lse, B, H, S, S, ldq=3 * vd, ldk=3 * vd, ldv=3 * vd, ldo=vd)
            xm = self.buf(tag + "xm", Mv, vd)
            self.linear(ctx, p + "o", xm, Mv, residual=x)
            st2 = self.buf(tag + "st2", 2, _rup(Mv, ROWPAD), torch.float32)
            a2, a2_8 = self.ln_q8(xm, p + "ln2", self.vit_eps, tag + "a2", Mv, st2[0], st2[1], Mv, p + "fc1", tag)
            z = self.buf(tag + "z", Mv, vf)
            # the GELU output's only reader is FFN-out: with a scale history it leaves the FFN-in epilogue as e4m3 bytes
            u8t = self.f8.target(p + "fc2.x", tag + "fc2.x", Mv, vf, E4M3) if self._fp8_ok(p + "fc2") else None
            u = self.buf(tag + "u", Mv, vf) if u8t is None else None
            u8 = self.linear(a2, p + "fc1", u, Mv, act=L.ACT_QUICK_GELU, zout=z, save_tag=tag if save else None, x8=a2_8, out8=u8t)
            xo = self.buf(f"v{l}.xo" if save else f"v_.xo{l & 1}", Mv, vd)
            self.linear(u, p + "fc2", xo, Mv, residual=xm, save_tag=tag if save else None, x8=u8 if u8t is not None else None)
            x = xo
        ehs = self.buf("v.ehs", Mv, P.d)
        self.linear(x, "vp", ehs, Mv)
        return x, ehs

    def vit_pooler(self, last: torch.Tensor, B: int) -> torch.Tensor:
        """pooler_output = post_layernorm(CLS) (only `encode()` exposes it; unused by captioning)."""
        P = self.P
        cls_rows = last[: B * P.S].view(B, P.S, P.vd)[:, 0].contiguous()
        out = torch.empty_like(cls_rows)
        ops.layernorm_fwd(cls_rows, P.f32("vit.post_ln.g"), P.f32("vit.post_ln.b"), self.vit_eps, out, rows=B)
        return out

    def vit_backward_bridge(self, B: int, dehs: torch.Tensor):
        """the part of vit_backward a frozen image tower still needs: the bridge's weight gradient and bias sum (`vp`), no dX — the
        ViT's layer backward, its LayerNorm / attention backward, vit_assemble_bwd and the patch-embedding dW do not run"""
        P = self.P
        Mv = B * P.S
        self.linear_bwd("vp", self.buf(f"v{P.vL - 1}.xo", Mv, P.vd), dehs, Mv, dx=None)

    def vit_backward(self, B: int, dehs: torch.Tensor):
        P = self.P
        S, vd, vf, H = P.S, P.vd, P.vffn, P.vH
        Mv, Mp = B * S, B * (S - 1)
        x_last = self.buf(f"v{P.vL - 1}.xo", Mv, vd)
        dx = self.dyb("vb.dx", P.vL - 1, Mv, vd)
        self.linear_bwd("vp", x_last, dehs, Mv, dx=dx)
        fp8 = self.fp8  # fp8 projections: their inputs exist as saved fp8 bytes (Fp8State.saved); the bf16 names below may hold nothing
        dx8 = None     # the Q8 of dx when the LayerNorm backward that produced it emitted the e5m2 bytes too
        for l in reversed(range(P.vL)):
            tag, p = f"v{l}.", f"vit{l}."
            qkv, ctx, xm = (self.buf(tag + n, Mv, c) for n, c in (("qkv", 3 * vd), ("ctx", vd), ("xm", vd)))
            a1, a2, u = ((None, None, None) if fp8 else (self.buf(tag + "a1", Mv, vd), self.buf(tag + "a2", Mv, vd), self.buf(tag + "u", Mv, vf)))
            z = self.buf(tag + "z", Mv, vf)
            st1, st2 = self.buf(tag + "st1", 2, _rup(Mv, ROWPAD), torch.float32), self.buf(tag + "st2", 2, _rup(Mv, ROWPAD), torch.float32)
            lse = self.vec(tag + "lse", B * H * S)
            x_in = self.buf(f"v{l - 1}.xo", Mv, vd) if l > 0 else self.buf("v.x0", Mv, vd)
            dz8t = self.dy8_target(p + "fc1", self._par(l), Mv)  # dz = dGELU-scaled dX of fc2 = the dy of fc1: e5m2 straight from the epilogue
            dz = self.dyb("vb.dz", l, Mv, vf) if dz8t is None else None
            self.linear_bwd(p + "fc2", u, dx, Mv, dx=dz, zin=z, dact=L.ACT_QUICK_GELU, defer=True, dy8=dx8, dx8=dz8t, par=self._par(l))
            da = self.buf("vb.da", Mv, vd)
            self.linear_bwd(p + "fc1", a2, dz, Mv, dx=da, defer=True, dy8=None if dz8t is None else dz8t.q8, par=self._par(l))
            dxm = self.dyb("vb.dxm", l, Mv, vd)
            self.ln_bwd("v2", l, xm, p + "ln2", st2[0], st2[1], da, dxm, Mv, dres=dx)
            dctx = self.buf("vb.dctx", Mv, vd)
            self.linear_bwd(p + "o", ctx, dxm, Mv, dx=dctx, defer=True)
            dq8t = None if packed_attn_tiled(S, S) else self.dy8_target(p + "qkv", self._par(l), Mv)
            if dq8t is not None:
                dqkv, q8 = None, dq8t.q
                grads = dict(grads8=(dq8t.out, dq8t.view(q8[:, vd:]).out, q8[:, 2 * vd:]))
            else:
                dqkv = self.dyb("vb.dqkv", l, Mv, 3 * vd)
                grads = dict(grads=(dqkv, dqkv[:, vd:], dqkv[:, 2 * vd:]), ldg=(3 * vd, 3 * vd, 3 * vd))
            self.attn_backward(qkv, qkv[:, vd:], qkv[:, 2 * vd:], ctx, dctx, lse, B, H, S, S, ldq=3 * vd, ldk=3 * vd, ldv=3 * vd, ldo=vd, lddo=vd,
                               **grads)
            self.linear_bwd(p + "qkv", a1, dqkv, Mv, dx=da, defer=True, dy8=None if dq8t is None else dq8t.q8, par=self._par(l))
            flush_now = self._dw_flush_layer(l)
            late = self.dw_fence() if flush_now else False
            if flush_now and not late:
                self.flush_dw()  # before LN1 backward overwrites dx (the fc2 gradient operand)
            dx = self.dyb("vb.dx", l - 1, Mv, vd)  # the layer below's residual-stream gradient (= its fc2 dW operand)
            # ... which the layer below's fc2 backward reads as e5m2: emitted here, beside the bf16 dx the residual path needs
            dx8t = self.dy8_target(f"vit{l - 1}.fc2", self._par(l - 1), Mv) if l > 0 else None
            if dx8t is not None:
                self.ln_bwd("v1", l, x_in, p + "ln1", st1[0], st1[1], da, dx, Mv, dres=dxm, q8=dx8t.out, q8_of_dx=True)
                dx8 = dx8t.q8
            else:
                self.ln_bwd("v1", l, x_in, p + "ln1", st1[0], st1[1], da, dx, Mv, dres=dxm)
                dx8 = None
            if flush_now and late:
                self.flush_dw(fence=False)
        emb = self.buf("v.emb", Mv, vd)
        st = self.buf("v.pre.stats", 2, _rup(Mv, ROWPAD), torch.float32)
        demb = self.buf("vb.demb", Mv, vd)
        self.ln_bwd("vpre", 0, emb, "vit.pre_ln", st[0], st[1], dx, demb, Mv)
        dpe = self.buf("vb.dpe", Mp, vd)
        ops.vit_assemble_bwd(demb, dpe, P.g("vit.cls"), P.g("vit.pos"), B, S, vd, vd)
        pk = P.ps * P.ps * 3
        patches = self.buf("v.patches", Mp, pk)
        ops.gemm(dpe, patches, P.g("patch.w"), vd, pk, _rup(Mp, ROWPAD), a_kmajor=True, b_kmajor=True)
        self._done("patch.w")

    # ------------------------------------------------------------------ decoder (teacher forced)
    def _kv_group(self, B: int, images, pack=None) -> int:
        """captions per image of a pass over B caption rows and `images` distinct images (None: B)"""
        if images is None or images == B:
            return 1
        if images < 1 or B % images:
            raise ValueError(f"{B} caption rows do not divide over {images} images")
        if self.fp8:
            raise ValueError("several captions per image are not supported together with fp8 GEMMs (the fused e5m2 emission of the "
                             "cross-attention's dK / dV has no shared form)")
        if pack is not None and len(pack) < 5:
            raise ValueError("packed rows with several captions per image: pack = (q_off, q_len, rows, q_off_img, q_len_img) — the last "
                             "two from train.group_packed_rows")
        return B // images

    def decoder_forward(self, ids, pos_ids, key_mask, ehs, B: int, T: int, save: bool, seed: Optional[int], pack=None, images=None):
        """ids/pos_ids/key_mask int32 [B*T]/[B*T]/[B,T]; ehs [images*S,d].  Returns final-layer-normed hidden [B*T,d].
        images (None = B): the number of distinct images — caption row r attends image r // (B // images); the cross k/v projections
        run at images*S rows and the cross-attention shares them (`attn_forward(kv_group=...)`).

        pack = (q_off int32 [B], q_len int32 [B], rows): PACKED rows — the decoder runs on the `rows` = sum(q_len) valid positions
        only (sequence b = rows [q_off[b], q_off[b] + q_len[b]); ids / pos_ids are then the packed arrays, key_mask is unused:
        every position of a sequence is valid).  Padded positions carry no loss (main.py:678) and no valid position attends to
        them (main.py:692: the labels' attention mask is the decoder's key mask), so everything they would compute or receive as
        gradient is exactly zero: leaving them out changes no result.  Buffers keep their [B*T] capacity."""
        P = self.P
        d, f, H, S = P.d, P.ffn, P.H, P.S
        G = self._kv_group(B, images, pack)
        Mcap, Mv = B * T, (B // G) * S
        M = pack[2] if pack is not None else Mcap  # rows the kernels process
        drop = seed is not None and self.p_drop > 0

        def sd(site):
            return _mix(seed, site) if drop else None

        h0 = self.buf("d.h0", Mcap, d)
        ops.embed_fwd(ids, pos_ids, P.w("shared"), P.f32("dec.pos"), self.embed_scale, h0, M, d)
        x = self.buf("d.x0", Mcap, d)
        ste = self.buf("d.emb.stats", 2, _rup(Mcap, ROWPAD), torch.float32)
        ops.layernorm_fwd(h0, P.f32("dec.ln_emb.g"), P.f32("dec.ln_emb.b"), self.dec_eps, x, ste[0], ste[1], rows=M,
                          dropout_p=self.p_drop if drop else 0.0, dropout_seed=sd(1) or 0)
        kvcat = self.cross_kv_all(ehs, Mv, "d." if save else "d_.", save) if self.ckv_hoisted() else None
        for l in range(P.L):
            tag = f"d{l}." if save else "d_."
            p = f"dec{l}."
            stats = self.buf(tag + "stats", 6, _rup(Mcap, ROWPAD), torch.float32)
            a, a8 = self.ln_q8(x, p + "ln_sa", self.dec_eps, tag + "a_sa", Mcap, stats[0], stats[1], M, p + "qkv", tag)
            qkv = self.buf(tag + "qkv", Mcap, 3 * d)
            self.linear(a, p + "qkv", qkv, M, save_tag=tag if save else None, x8=a8)
            ctx = self.buf(tag + "ctx", Mcap, d)
            lse = self.vec(tag + "lse", B * H * T)
            self.attn_forward(qkv, qkv[:, d:], qkv[:, 2 * d:], ctx, lse, B, H, T, T, ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d, pack=pack,
                              kv_packed=True, key_mask=key_mask, causal=True)
            x1 = self.buf(tag + "x1", Mcap, d)
            self.linear(ctx, p + "so", x1, M, residual=x, drop_seed=sd(10 + 3 * l))
            a, a8 = self.ln_q8(x1, p + "ln_ca", self.dec_eps, tag + "a_ca", Mcap, stats[2], stats[3], M, p + "cq", tag)
            q = self.buf(tag + "cq", Mcap, d)
            self.linear(a, p + "cq", q, M, save_tag=tag if save else None, x8=a8)
            if kvcat is not None:
                kv, ldkv = kvcat[:, l * 2 * d:], kvcat.stride(0)
            else:
                kv, ldkv = self.buf(tag + "ckv", Mv, 2 * d), 2 * d
                self.linear(ehs, p + "ckv", kv, Mv, save_tag="d.ehs." if save else None, stable_input=True)
            cctx = self.buf(tag + "cctx", Mcap, d)
            clse = self.vec(tag + "clse", B * H * T)
            self.attn_forward(q, kv, kv[:, d:], cctx, clse, B, H, T, S, ldq=d, ldk=ldkv, ldv=ldkv, ldo=d, pack=pack, kv_group=G)
            x2 = self.buf(tag + "x2", Mcap, d)
            self.linear(cctx, p + "co", x2, M, residual=x1, drop_seed=sd(11 + 3 * l))
            a, a8 = self.ln_q8(x2, p + "ln_ff", self.dec_eps, tag + "a_ff", Mcap, stats[4], stats[5], M, p + "fc1", tag)
            z = self.buf(tag + "z", Mcap, f)
            u8t = self.f8.target(p + "fc2.x", tag + "fc2.x", Mcap, f, E4M3) if self._fp8_ok(p + "fc2") else None
            u = self.buf(tag + "u", Mcap, f) if u8t is None else None
            u8 = self.linear(a, p + "fc1", u, M, act=self.gelu, zout=z, save_tag=tag if save else None, x8=a8, out8=u8t)
            x3 = self.buf(f"d{l}.x3" if save else f"d_.x3{l & 1}", Mcap, d)
            self.linear(u, p + "fc2", x3, M, residual=x2, drop_seed=sd(12 + 3 * l), save_tag=tag if save else None,
                        x8=u8 if u8t is not None else None)
            x = x3
        hf = self.buf("d.hf", Mcap, d)
        stf = self.buf("d.f.stats", 2, _rup(Mcap, ROWPAD), torch.float32)
        ops.layernorm_fwd(x, P.f32("dec.ln_f.g"), P.f32("dec.ln_f.b"), self.dec_eps, hf, stf[0], stf[1], rows=M)
        return hf

    # ------------------------------------------------------------------ cross-attention k/v of all layers as one GEMM
    def ckv_hoisted(self) -> bool:
        """the cross-attention k/v projections of all decoder layers run as ONE GEMM each way (forward, dX, dW): they read the
        same encoder states and their weights sit side by side (ParamStore.ckv_cat).  L one-round launches (3200 x 2048 x 1024:
        400 tiles of 128x128) become one with 1248 tiles of 256x256; the dX sum over the layers becomes a K = L*2d contraction
        with one rounding instead of L bf16 accumulations.  fp8 mode: the same three launches on fp8 operands, the concatenated
        weight and the concatenated k/v gradient each under ONE scale.  MIC_CKV_HOIST=0 switches back (A/B)."""
        return self._ckv_hoist

    def cross_kv_all(self, ehs, Mv: int, tag: str, save: bool = False):
        """[Mv][L*2d]: layer l's (k | v) in columns [l*2d, (l+1)*2d)"""
        P = self.P
        w, b = P.ckv_cat("w")
        kvcat = self.buf(tag + "ckvcat", Mv, P.L * 2 * P.d)
        if self.fp8 and "ckvcat" in self.f8.weights:
            f8 = self.f8
            f8.wait()
            w8 = f8.weights["ckvcat"]
            x8 = f8.quant(ehs, Mv, P.d, "ckvcat.x", tag + "ckvcat.x", E4M3)
            if save:
                f8.saved["ckvcat"] = x8
            ops.gemm(x8.q, w8.q, kvcat, Mv, P.L * 2 * P.d, P.d, bias=b, a_scale_inv=x8.scale_inv, b_scale_inv=w8.scale_inv)
        else:
            ops.gemm(ehs, w, kvcat, Mv, P.L * 2 * P.d, P.d, bias=b)
        return kvcat

    def head_logits(self, hf, M: int, name: str = "d.logits", stats: bool = False, fp8: bool = False, shortlist: Optional[Shortlist] = None):
        """Tied head (modeling:170-178): logits[M, Vpad] = hf @ shared^T + final_logits_bias (compute dtype).
        stats=True (bf16 mode): also returns the GEMM's softmax partials per 64-column granule [M][Vpad/64][2] (fp32) so that the
        log-softmax downstream (cross-entropy, beam scores) needs no second pass over the logits.
        shortlist (up to date: Shortlist.refresh): the same GEMM over the shortlist's gathered rows only — logits [M, Ns_pad], column c =
        token shortlist.map[c], partials over the Ns valid columns — into buffers of their own (the full-vocabulary ones are untouched)."""
        P = self.P
        if shortlist is not None:
            sl = shortlist
            logits = self.buf(name + ".sl", M, sl.Ns_pad)
            stat = None
            if stats and self.dt == torch.bfloat16 and self.use_head_stats:
                stat = self.buf(name + ".sl.stat", M, 2 * (sl.Ns_pad // 64), torch.float32)
            ops.gemm(hf, sl.E, logits, M, sl.Ns_pad, P.d, bias=sl.bias, rowstat=stat, rowstat_nvalid=sl.Ns)
            return (logits, stat) if stats else logits
        logits = self.buf(name, M, P.Vpad)
        stat = self.head_stats(name, M) if stats else None
        self._head_project(hf, logits, M, stat, fp8=fp8)  # (fp8: the train / eval passes only — inference stays in the storage dtype)
        return (logits, stat) if stats else logits

    def _head8(self) -> bool:
        return self.fp8 and self.fp8_head > 0

    def _head_project(self, hf, logits, M: int, stat, fp8: bool = True):
        """logits[:M] = hf[:M] @ shared^T + final_logits_bias (+ the softmax partials): bf16 operands, or — fp8 GEMMs with
        MIC_FP8_HEAD=all — the e4m3 copies of both (the quantised hidden states stay for the head's weight gradient)"""
        P = self.P
        if fp8 and self._head8() and self.fp8_head == 2:
            f8 = self.f8
            x8 = f8.head_x = f8.quant(hf, M, P.d, "head.x", "head.x", E4M3)
            E8 = f8.weights["shared"]
            f8.wait()
            ops.gemm(x8.q, E8.q, logits, M, P.Vpad, P.d, bias=P.f32("flb"), rowstat=stat, rowstat_nvalid=P.V,
                     a_scale_inv=x8.scale_inv, b_scale_inv=E8.scale_inv)
        else:
            ops.gemm(hf, P.w("shared"), logits, M, P.Vpad, P.d, bias=P.f32("flb"), rowstat=stat, rowstat_nvalid=P.V)

    def head_stats(self, name: str, M: int):
        if self.dt != torch.bfloat16 or not self.use_head_stats:
            return None  # the fp32 (parity) GEMM kernel has no by-products: its consumers stream the logits
        return self.buf(name + ".stat", M, 2 * (self.P.Vpad // 64), torch.float32)  # (max, sum exp) per 64-column granule

    def decoder_backward(self, B: int, T: int, ids, pos_ids, key_mask, ehs, dlogits, seed: Optional[int], rows=None, pack=None, images=None):
        """Consumes dlogits [M,Vpad] (or [Mc,Vpad] for the compacted head: rows = (idx int32 [Mc], Mc)); writes all
        decoder/embedding/head grads; returns dehs [images*S,d].  pack: see decoder_forward (the compacted head's rows ARE the packed
        rows then: no gather / scatter between the head and the decoder).  images: see decoder_forward — dK / dV of the cross-attention
        arrive summed over an image's captions, so the ckv dX / dW GEMMs and dehs have images*S rows."""
        P = self.P
        d, f, H, S = P.d, P.ffn, P.H, P.S
        G = self._kv_group(B, images, pack)
        Mcap, Mv = B * T, (B // G) * S
        M = pack[2] if pack is not None else Mcap
        drop = seed is not None and self.p_drop > 0
        pd = self.p_drop if drop else 0.0

        def sd(site):
            return _mix(seed, site) if drop else 0

        dhf = self.buf("db.dhf", Mcap, d)
        if rows is None:
            hf = self.buf("d.hf", Mcap, d)
            Mh = M
        else:
            hf = self.buf("d.hf" if pack is not None else "d.hfc", Mcap, d)  # compacted final hidden states (pad rows zero)
            Mh = rows[1]
        Mhp = _rup(Mh, 64)
        nt = self._head_nt_state
        self._head_nt_state = None
        f8 = self.f8 if self.fp8 else None
        h8s = None
        if f8 is not None:
            h8s, f8.head_dy = f8.head_dy, None
        if h8s is not None:
            dl8, coef, labels = h8s
            # fp8 head: dE = dlogits^T . h over K = rows, both operands k-major (the e5m2 copy of dlogits as the CE backward wrote it,
            # the e4m3 hidden states; rows >= Mh of the 128-row reduction padding count as zero), fp32 straight into the gradient buffer
            x8 = f8.head_x or f8.quant(hf, Mh, d, "head.x", "head.x", E4M3)
            ops.gemm(dl8.q, x8.q, P.g("shared"), P.Vpad, d, _rup(Mh, 128), a_kmajor=True, b_kmajor=True, k_valid=Mh,
                     a_scale_inv=dl8.scale_inv, b_scale_inv=x8.scale_inv)
            # the label entries (kept out of the byte matrix): + coef h into dE's label rows, coef E[label] as one more slab of dX
            tiles = ((Mh + 255) // 256) * ((d + 255) // 256)
            nsp = max(1, min(ops.get_cu_budget() // tiles, P.Vpad // 128 // 2))
            slab_rows = _rup(Mh, 256)
            cap_rows = max(_rup(Mcap, 256), (256 // max(1, (d + 255) // 256)) * 256) + _rup(Mcap, 256)
            d32 = self.buf("db.dhf32", cap_rows, d, torch.float32)
            assert (nsp + 1) * slab_rows <= d32.shape[0], (nsp, slab_rows, d32.shape)
            ops.head_label_terms(labels, coef, P.w("shared"), hf, d32[nsp * slab_rows:], P.g("shared"), Mh, d)
        elif nt is not None:
            # NT launches on the four-wave kernel: dE = dlogits^T . (h^T)^T over K = rows (zero-padded to a multiple of 128 by the CE
            # backward; the bias gradient was summed there), fp32 straight into the gradient buffer
            dT, Kp = nt
            hfT = self.buf("d.hfT", d, dT.shape[1])
            ops.transpose_bf16(hf, hfT, Mh, d, rows_pad=Kp)
            ops.gemm(dT, hfT, P.g("shared"), P.Vpad, d, Kp)
        elif self.dt == torch.bfloat16:  # final_logits_bias gradient = row sums of dlogits^T, fused into the dE GEMM
            ops.zero(P.g("flb"))        # (atomics; this segment sits in front of the pre-zeroed atomic region)
            ops.gemm(dlogits, hf, P.g("shared"), P.Vpad, d, Mhp, a_kmajor=True, b_kmajor=True, a_rowsum=P.g("flb"), rowsum_k=Mh)
        else:
            ops.colsum(dlogits, P.g("flb"), Mh, P.Vpad, dlogits.stride(0))
            ops.gemm(dlogits, hf, P.g("shared"), P.Vpad, d, Mhp, a_kmajor=True, b_kmajor=True)
        # dense (LM head) part of the tied embedding gradient: the first thing backward completes — its exchange starts here.  The
        # dX GEMM below still READS the embedding: the Trainer's reducer issues this bucket's optimizer pass at the next progress
        # report, behind it (GradReducer `defer`)
        self._done("shared")
        dhc = dhf if (rows is None or pack is not None) else self.buf("db.dhfc", Mcap, d)
        if h8s is not None:
            # dX = dlogits . (E^T)^T over K = Vpad on the e5m2 / e4m3 copies, split over K as below; the slabs and the label slab are
            # summed and rounded to bf16 once
            E8 = f8.weights["shared"]
            f8.wait()
            slab = slab_rows * d
            ops.gemm(dl8.q, E8.qT, d32, Mh, d, P.Vpad, split_k=nsp, split_stride=slab if nsp > 1 else 0, a_scale_inv=dl8.scale_inv, b_scale_inv=E8.scale_inv)
            ops.sum_slabs(d32, nsp + 1, slab, dhc, Mh, d, d32.stride(0), dhc.stride(0))
        elif nt is not None:
            # dX = dlogits . (E^T)^T over K = Vpad: ceil(Mh / 256) x d / 256 output tiles, split over K so that one round of blocks
            # fills the chip; one fp32 slab per split, summed and rounded to bf16 once
            tiles = ((Mh + 255) // 256) * ((d + 255) // 256)
            nsp = max(1, min(ops.get_cu_budget() // tiles, P.Vpad // 128 // 2))
            # ONE workspace whatever this batch's row count: a slab is as tall as the valid rows (rounded to the tile), and
            # nsp * slab rows <= budget / (d / 256) tile rows — a buffer keyed on nsp would add ~100 MB per distinct split seen
            # during training on ragged batches.  (The split itself follows Mh: the fp32 summation order of dX is a function of
            # the batch's row count, like every tile choice of the planner.)
            slab_rows = _rup(Mh, 256)
            cap_rows = max(_rup(Mcap, 256), (256 // max(1, (d + 255) // 256)) * 256)
            d32 = self.buf("db.dhf32", cap_rows, d, torch.float32)
            assert nsp * slab_rows <= d32.shape[0], (nsp, slab_rows, d32.shape)
            slab = slab_rows * d
            ops.gemm(dlogits, self.shared_T(), d32, Mh, d, P.Vpad, split_k=nsp, split_stride=slab if nsp > 1 else 0)
            if nsp > 1:
                ops.sum_slabs(d32, nsp, slab, dhc, Mh, d, d32.stride(0), dhc.stride(0))
            else:
                ops.cast2d(d32, dhc, Mh, d, d32.stride(0), dhc.stride(0))
        elif self.dt == torch.bfloat16 and P.Vpad >= 16384:
            # [Mh, d] output, reduction over the whole vocabulary: far too few tiles to fill 256 CUs.  Split-K 32 with K-range
            # <-> XCD affinity (gemm.hip) into per-split fp32 slabs (no atomics), summed and rounded to bf16 once.
            nsp = 32  # 16..64 measure the same (+-0.1 ms/step); the gain over the atomic variant is the absence of atomics
            d32 = self.buf("db.dhf32", nsp * _rup(Mcap, ROWPAD), d, torch.float32)  # one fp32 slab per split, summed below
            slab = _rup(Mcap, ROWPAD) * d
            ops.gemm(dlogits, P.w("shared"), d32, Mh, d, P.Vpad, b_kmajor=True, split_k=nsp, split_stride=slab)
            ops.sum_slabs(d32, nsp, slab, dhc, Mh, d, d32.stride(0), dhc.stride(0))
        else:
            ops.gemm(dlogits, P.w("shared"), dhc, Mh, d, P.Vpad, b_kmajor=True)
        if rows is not None and pack is None:
            ops.zero(dhf[:M])  # masked-out positions receive exactly zero gradient from the loss
            ops.copy_rows(dhc, dhf, Mh, d, dst_idx=rows[0])
        dx = self.buf("db.dx", Mcap, d)
        # masked gradients entering the FFN / cross-attention / self-attention branches and the other operands of the deferred
        # weight-gradient GEMMs come from dyb(): one buffer per layer parity while dW runs on its own stream
        stf = self.buf("d.f.stats", 2, _rup(Mcap, ROWPAD), torch.float32)
        x_last = self.buf(f"d{P.L - 1}.x3", Mcap, d)
        # dxm: the dropout-masked residual-stream gradient = the dy of the top layer's FFN-out projection, its only reader: with a
        # scale history it leaves the LayerNorm backward as e5m2 bytes only
        dxm8t = self.dy8_target(f"dec{P.L - 1}.fc2", self._par(P.L - 1), Mcap)
        dxm = self.dyb("db.dxm_a", P.L - 1, Mcap, d) if dxm8t is None else None
        self.ln_bwd("f", 0, x_last, "dec.ln_f", stf[0], stf[1], dhf, dx, M, dxm=dxm, dropout_p=pd, dropout_seed=sd(12 + 3 * (P.L - 1)),
                    **({} if dxm8t is None else dict(q8=dxm8t.out)))
        dxm8 = None if dxm8t is None else dxm8t.q8
        dehs = self.buf("db.dehs", Mv, d)
        hoist = self.ckv_hoisted()
        kvcat = self.buf("d.ckvcat", Mv, P.L * 2 * d) if hoist else None
        hoist8 = hoist and f8 is not None and "ckvcat" in f8.weights
        # fp8, hoisted: every layer's dK | dV lands in its column slice of ONE e5m2 matrix under one scale (fused emission) ...
        dkvcat8t = f8.target("ckvcat.dy", "f8.ckvcat.dy", Mv, P.L * 2 * d, E5M2) if (hoist8 and not packed_attn_tiled(T, S)) else None
        # ... or, without a scale history, in the bf16 matrix that is quantised once behind the loop
        dkvcat = self.buf("db.dkvcat", Mv, P.L * 2 * d) if (hoist and dkvcat8t is None) else None
        for l in reversed(range(P.L)):
            tag, p = f"d{l}.", f"dec{l}."
            stats = self.buf(tag + "stats", 6, _rup(Mcap, ROWPAD), torch.float32)
            qkv, ctx, x1 = (self.buf(tag + n, Mcap, c) for n, c in (("qkv", 3 * d), ("ctx", d), ("x1", d)))
            cq, cctx, x2 = (self.buf(tag + n, Mcap, d) for n in ("cq", "cctx", "x2"))
            ckv, ldkv = (kvcat[:, l * 2 * d:], kvcat.stride(0)) if hoist else (self.buf(tag + "ckv", Mv, 2 * d), 2 * d)
            z = self.buf(tag + "z", Mcap, f)
            # (fp8 projections read their saved fp8 inputs, Fp8State.saved: the bf16 copies need not exist)
            a_sa, a_ca, a_ff, u = (None,) * 4 if f8 is not None else (self.buf(tag + "a_sa", Mcap, d), self.buf(tag + "a_ca", Mcap, d),
                                                          self.buf(tag + "a_ff", Mcap, d), self.buf(tag + "u", Mcap, f))
            lse, clse = self.vec(tag + "lse", B * H * T), self.vec(tag + "clse", B * H * T)
            x_in = self.buf(f"d{l - 1}.x3", Mcap, d) if l > 0 else self.buf("d.x0", Mcap, d)
            # --- FFN branch: x3 = x2 + drop(fc2(gelu(fc1(LN(x2)))));  dxm = dropout-masked dx3
            dxm_b, dxm_c = self.dyb("db.dxm_b", l, Mcap, d), self.dyb("db.dxm_c", l, Mcap, d)
            dz8t = self.dy8_target(p + "fc1", self._par(l), Mcap)
            dz = self.dyb("db.dz", l, Mcap, f) if dz8t is None else None
            self.linear_bwd(p + "fc2", u, dxm, M, dx=dz, zin=z, dact=self.gelu, defer=True, dy8=dxm8, dx8=dz8t, par=self._par(l))
            da = self.buf("db.da", Mcap, d)
            self.linear_bwd(p + "fc1", a_ff, dz, M, dx=da, defer=True, dy8=None if dz8t is None else dz8t.q8, par=self._par(l))
            dx2 = self.buf("db.dx2", Mcap, d)
            self.ln_bwd("ff", l, x2, p + "ln_ff", stats[4], stats[5], da, dx2, M,
                        dres=dx, dxm=dxm_b, dropout_p=pd, dropout_seed=sd(11 + 3 * l))
            # --- cross-attention branch
            dctx = self.buf("db.dctx", Mcap, d)
            self.linear_bwd(p + "co", cctx, dxm_b, M, dx=dctx, defer=True)
            one_tile = not packed_attn_tiled(T, S)
            dq8t = self.dy8_target(p + "cq", self._par(l), Mcap) if one_tile else None
            if hoist:
                dkv8t = None if dkvcat8t is None else dkvcat8t.view(dkvcat8t.q[:, l * 2 * d:])
            else:
                dkv8t = self.dy8_target(p + "ckv", self._par(l), Mv) if one_tile else None
            if dq8t is not None and dkv8t is not None:
                # dQ [rows][d] and dK | dV [encoder rows][2d] as e5m2 bytes under their own scales, straight out of the attention backward
                dq, dkv, dq8, dkv8 = None, None, dq8t.q8, dkv8t.q8
                grads = dict(grads8=(dq8t.out, dkv8t.out, dkv8t.q[:, d:]))
            elif hoist and dkvcat8t is not None:
                # (dQ has no scale history yet but the concatenated k/v gradient has: cannot happen after the first pass; keep the bytes consistent)
                raise RuntimeError("fp8: cross-attention dQ without a scale history beside a hoisted k/v gradient with one")
            else:
                dq, dq8, dkv8 = self.dyb("db.dq", l, Mcap, d), None, None
                dkv = dkvcat[:, l * 2 * d:] if hoist else self.dyb("db.dkv", l, Mv, 2 * d)
                grads = dict(grads=(dq, dkv, dkv[:, d:]), ldg=(d, ldkv, ldkv))
            self.attn_backward(cq, ckv, ckv[:, d:], cctx, dctx, clse, B, H, T, S, ldq=d, ldk=ldkv, ldv=ldkv, ldo=d, lddo=d, pack=pack, kv_group=G,
                               **grads)
            self.linear_bwd(p + "cq", a_ca, dq, M, dx=da, defer=True, dy8=dq8, par=self._par(l))
            if not hoist:
                self.linear_bwd(p + "ckv", ehs, dkv, Mv, dx=dehs, dx_accumulate=(l != P.L - 1), defer=True, dy8=dkv8, par=self._par(l))
            dx1 = self.buf("db.dx1", Mcap, d)
            self.ln_bwd("ca", l, x1, p + "ln_ca", stats[2], stats[3], da, dx1, M,
                        dres=dx2, dxm=dxm_c, dropout_p=pd, dropout_seed=sd(10 + 3 * l))
            # --- self-attention branch
            self.linear_bwd(p + "so", ctx, dxm_c, M, dx=dctx, defer=True)
            dqkv8t = None if packed_attn_tiled(T, T) else self.dy8_target(p + "qkv", self._par(l), Mcap)
            if dqkv8t is not None:
                dqkv, q8 = None, dqkv8t.q
                grads = dict(grads8=(dqkv8t.out, dqkv8t.view(q8[:, d:]).out, q8[:, 2 * d:]))
            else:
                dqkv = self.dyb("db.dqkv", l, Mcap, 3 * d)
                grads = dict(grads=(dqkv, dqkv[:, d:], dqkv[:, 2 * d:]), ldg=(3 * d, 3 * d, 3 * d))
            self.attn_backward(qkv, qkv[:, d:], qkv[:, 2 * d:], ctx, dctx, lse, B, H, T, T, ldq=3 * d, ldk=3 * d, ldv=3 * d, ldo=d, lddo=d, pack=pack,
                               kv_packed=True, key_mask=key_mask, causal=True, **grads)
            self.linear_bwd(p + "qkv", a_sa, dqkv, M, dx=da, defer=True, dy8=None if dqkv8t is None else dqkv8t.q8, par=self._par(l))
            flush_now = self._dw_flush_layer(l)
            late = self.dw_fence() if flush_now else False
            if flush_now and not late:
                self.flush_dw()  # the layer's 7 weight-gradient GEMMs as one grouped launch (before dxm_a is rewritten)
            if l > 0:
                dxm8t = self.dy8_target(f"dec{l - 1}.fc2", self._par(l - 1), Mcap)
                dxm = self.dyb("db.dxm_a", l - 1, Mcap, d) if dxm8t is None else None
                self.ln_bwd("sa", l, x_in, p + "ln_sa", stats[0], stats[1], da, dx, M, dres=dx1, dxm=dxm, dropout_p=pd,
                            dropout_seed=sd(12 + 3 * (l - 1)), **({} if dxm8t is None else dict(q8=dxm8t.out)))
                dxm8 = None if dxm8t is None else dxm8t.q8
            else:
                self.ln_bwd("sa", l, x_in, p + "ln_sa", stats[0], stats[1], da, dx, M, dres=dx1)
            if flush_now and late:
                self.flush_dw(fence=False)
        if hoist:
            # the cross-attention k/v projections of all layers at once: dW (+ bias row sums) = dkv^T ehs as one [L*2d][d] weight
            # gradient (on the dW stream), dehs = dkv W as one contraction over K = L*2d (split over K into fp32 slabs: 52 output
            # tiles of 256x256 cannot fill the chip)
            wcat, _ = P.ckv_cat("w")
            gw, gb = P.ckv_cat("g")
            N = P.L * 2 * d
            Mvp = _rup(Mv, ROWPAD)
            if hoist8:
                dkv8 = dkvcat8t.q8 if dkvcat8t is not None else f8.quant(dkvcat, Mv, N, "ckvcat.dy", "f8.ckvcat.dy", E5M2)
                x8 = f8.saved.get("ckvcat")
                if x8 is None:
                    raise RuntimeError("fp8 backward of the hoisted cross k/v projection: the forward pass did not keep the fp8 encoder states")
                w8 = f8.weights["ckvcat"]
                nsp = min(8, N // 128)
                if nsp > 1:
                    slab = Mvp * d
                    d32 = self.buf("db.dehs32", nsp * Mvp, d, torch.float32)
                    ops.gemm(dkv8.q, w8.qT, d32, Mv, d, N, split_k=nsp, split_stride=slab, a_scale_inv=dkv8.scale_inv, b_scale_inv=w8.scale_inv)
                    ops.sum_slabs(d32, nsp, slab, dehs, Mv, d, d32.stride(0), dehs.stride(0))
                else:
                    ops.gemm(dkv8.q, w8.qT, dehs, Mv, d, N, a_scale_inv=dkv8.scale_inv, b_scale_inv=w8.scale_inv)
                self._dw8_queue.append((ops.gemm_args(dkv8.q, x8.q, gw, N, d, Mvp, a_kmajor=True, b_kmajor=True, k_valid=Mv,
                                                      a_scale_inv=dkv8.scale_inv, b_scale_inv=x8.scale_inv), f"dec{P.L - 1}.ckv", True))
                self._cs8_queue.append((dkv8.q, gb, dkv8.scale_inv, Mv, N))
                self._ckv_block_name = f"dec{P.L - 1}.ckv"
                try:
                    self.flush_dw()
                finally:
                    self._ckv_block_name = None
            else:
                # (bf16 / fp32 operands)
                fuse = self.dt == torch.bfloat16
                rs = dict(a_rowsum=gb, rowsum_k=Mv) if fuse else {}
                # dX first: it READS the weights, and reporting their gradients final (flush_dw -> _done) lets the per-bucket optimizer
                # rewrite them; the dW stream's launch waits for everything enqueued here, so the bucket's event covers this GEMM too
                nsp = min(8, N // 64)  # K-tiles of 64: a reduced model may have fewer than 8 of them
                if self.dt == torch.bfloat16 and nsp > 1:
                    slab = Mvp * d
                    d32 = self.buf("db.dehs32", nsp * Mvp, d, torch.float32)
                    ops.gemm(dkvcat, wcat, d32, Mv, d, N, b_kmajor=True, split_k=nsp, split_stride=slab)
                    ops.sum_slabs(d32, nsp, slab, dehs, Mv, d, d32.stride(0), dehs.stride(0))
                else:
                    ops.gemm(dkvcat, wcat, dehs, Mv, d, N, b_kmajor=True)
                self._dw_queue.append((ops.gemm_args(dkvcat, ehs, gw, N, d, Mvp, a_kmajor=True, b_kmajor=True, **rs), f"dec{P.L - 1}.ckv", True))
                if not fuse:
                    self._cs_queue.append((dkvcat, gb, Mv, N, dkvcat.stride(0)))
                self._ckv_block_name = f"dec{P.L - 1}.ckv"
                try:
                    self.flush_dw()
                finally:
                    self._ckv_block_name = None
        else:
            # per-layer k/v projections: every layer's dW GEMM (and the dX GEMMs that read these weights) has been issued by now
            self._done(f"dec{P.L - 1}.ckv.w")
        # embedding LayerNorm (+ its dropout) and the token/position embedding scatter
        h0 = self.buf("d.h0", Mcap, d)
        ste = self.buf("d.emb.stats", 2, _rup(Mcap, ROWPAD), torch.float32)
        dh0 = self.buf("db.dh0", Mcap, d)
        self.ln_bwd("emb", 0, h0, "dec.ln_emb", ste[0], ste[1], dx, dh0, M,
                    in_dropout_p=pd, in_dropout_seed=sd(1))
        if self.defer_embed:
            ops.embed_bwd(ids, pos_ids, dh0, self.embed_scale, None, P.g("dec.pos"), M, d)
            # the ranks exchange a FIXED number of (id, dh0) rows and add them up deterministically (mic_embed_rows_add_det: the
            # replicas must stay bit-identical): rows that carry no gradient — behind this rank's valid packed rows, or at padded
            # positions (their dh0 is exactly zero) — travel with id -1 and are skipped
            n_x = Mcap if pack is not None else M
            ids_x = self.vec("db.ids_x", Mcap, torch.int32)
            ids_x[:n_x].copy_(ids[:n_x])
            if pack is not None:
                if M < Mcap:
                    ids_x[M:Mcap].fill_(-1)
            elif key_mask is not None:
                ids_x[:n_x].masked_fill_(key_mask.reshape(-1)[:n_x] == 0, -1)
            self.embed_rows = (ids_x, dh0, n_x)
        else:
            # single process: the scatter lands before the optimizer touches the segment (Trainer holds that bucket)
            ops.embed_bwd(ids, pos_ids, dh0, self.embed_scale, P.g("shared"), P.g("dec.pos"), M, d)
            if self.on_embed_rows is not None:
                self.on_embed_rows()  # the tied embedding's gradient is complete (dense head part + these rows): its late optimizer pass may go
        return dehs

    # ------------------------------------------------------------------ loss (main.py:658-680) on materialised logits
    def loss_and_dlogits(self, logits, labels, mask, M: int, label_smoothing: float, backward: bool, stat=None, row_weights=None):
        """row_weights (fp32 device vector, one per head row; None: the plain loss): loss = sum w mask row_loss / sum mask, and the
        weight enters dlogits through the row factor (mic_ce_reduce_w / mic_ce_bwd_w / mic_ce_bwd_t_w) — everything behind the
        cross-entropy is linear in it.  Refused with fp8 GEMMs (mic_ce_bwd_q8's closed-form scale rests on |g| <= 1)."""
        P = self.P
        self._check_row_weights(row_weights, M)
        lse, rl = self.vec("ce.lse", _rup(M, ROWPAD)), self.vec("ce.rowloss", _rup(M, ROWPAD))
        loss, denom = self.vec("ce.loss", 1), self.vec("ce.denom", 1)
        if stat is not None and label_smoothing == 0.0:
            ops.ce_rows_tiles(logits, logits.stride(0), P.V, stat, labels, lse, rl, M)  # lse from the head GEMM's tile partials
        else:
            ops.ce_rows(logits, logits.stride(0), P.V, labels, mask, label_smoothing, lse, rl, M)
        if row_weights is None:
            ops.ce_reduce(rl, mask, loss, denom, M)
        else:
            ops.ce_reduce(rl, mask, loss, denom, M, row_weight=row_weights)
        if backward and self._head8():
            # fp8 head: dlogits leave as ONE e5m2 copy (the logits stay) under the scale this tensor has in closed form (mic_ce_bwd_q8)
            ops.zero(P.g("flb"))
            q = self.buf("head.dl.q8", logits.shape[0], P.Vpad, E5M2)
            st = self.vec("head.dl.state", 2)
            # ... except the label entry of every row (at least half of the row's gradient energy): an fp32 coefficient whose two
            # products decoder_backward adds exactly (mic_head_label_terms)
            coef = self.vec("head.dl.coef", _rup(logits.shape[0], ROWPAD))
            ops.ce_bwd_q8(logits, logits.stride(0), P.V, P.Vpad, labels, mask, label_smoothing, lse, denom, M, ops.fp8_out(q, st), colsum=P.g("flb"),
                          label_coef=coef)
            self.f8.head_dy = (Q8(q, st), coef, labels)
            self._head_nt_state = None
        elif backward:
            kcap = self._head_nt_kcap(logits)
            if kcap:
                # dlogits in place AND transposed [Vpad][Kp] (reduction padding rows M .. Kp zero), final_logits_bias gradient on the way
                Kp = _rup(M, 128)
                dT = self.buf("d.dlogitsT", P.Vpad, kcap)
                ops.zero(P.g("flb"))
                if row_weights is None:
                    ops.ce_bwd_t(logits, logits.stride(0), P.V, P.Vpad, labels, mask, label_smoothing, lse, denom, M, dT, rows_pad=Kp, colsum=P.g("flb"))
                else:
                    ops.ce_bwd_t(logits, logits.stride(0), P.V, P.Vpad, labels, mask, label_smoothing, lse, denom, M, dT, rows_pad=Kp, colsum=P.g("flb"),
                                 row_weight=row_weights)
                self._head_nt_state = (dT, Kp)
            else:
                if row_weights is None:
                    ops.ce_bwd(logits, logits.stride(0), P.V, P.Vpad, labels, mask, label_smoothing, lse, denom, M)
                else:
                    ops.ce_bwd(logits, logits.stride(0), P.V, P.Vpad, labels, mask, label_smoothing, lse, denom, M, row_weight=row_weights)
                self._head_nt_state = None
        return loss

    def _check_row_weights(self, row_weights, n: int):
        """per-row loss weights of a pass whose head has `n` rows: checked before anything is launched (None: nothing to check)"""
        if row_weights is None:
            return
        if self.fp8:
            raise ValueError("row_weights are not supported together with fp8 GEMMs (out of scope: the e5m2 dlogits of mic_ce_bwd_q8 "
                             "carry a closed-form scale that rests on |g| <= 1)")
        if (not isinstance(row_weights, torch.Tensor) or row_weights.dtype != torch.float32 or row_weights.dim() != 1
                or row_weights.numel() != n or not row_weights.is_contiguous() or row_weights.device.type != self.dev.type):
            raise ValueError(f"row_weights: a contiguous float32 vector of {n} elements on {self.dev} (one per head row), got "
                             f"{getattr(row_weights, 'dtype', type(row_weights))} {tuple(getattr(row_weights, 'shape', ()))}")

    def _head_nt_kcap(self, logits) -> int:
        """columns of the dlogits^T buffer (the capacity of the row dimension, a multiple of 128) when the head's backward runs as NT
        launches of the four-wave kernel, else 0: bf16 storage, a vocabulary worth the copies, operands inside the 2^31-byte
        window that kernel's buffer resources address"""
        P = self.P
        if not self.head_nt or self.dt != torch.bfloat16 or P.Vpad < 16384 or P.d % 128 != 0 or self._head8():
            return 0
        kcap = _rup(logits.shape[0], 128)
        return kcap if P.Vpad * kcap * 2 < 0x7fffffff and logits.shape[0] * logits.stride(0) * 2 < 0x7fffffff else 0

    def shared_T(self):
        """E^T [d][Vpad] (bf16): the k-contiguous copy of the tied embedding that the head's dX GEMM streams (dX = dlogits E reduces
        over the vocabulary).  Rebuilt when the weights changed (ParamStore.version) — by the Trainer on a side stream behind its
        optimizer passes (`refresh_shared_T`), here on the spot otherwise."""
        P = self.P
        ET = self.buf("w.sharedT", P.d, P.Vpad)
        ver = getattr(P, "version", 0)
        if self._ET_version != ver:
            if self._ET_event is not None:  # a side-stream refresh of an older version may still be writing this buffer
                torch.cuda.current_stream().wait_event(self._ET_event)
            ops.transpose_bf16(P.w("shared"), ET, P.Vpad, P.d)
            self._ET_version, self._ET_event = ver, None
        elif self._ET_event is not None:
            torch.cuda.current_stream().wait_event(self._ET_event)
            self._ET_event = None
        return ET

    def refresh_shared_T(self, side, version: int):
        """Trainer, end of a step: rebuild E^T from the updated embedding on `side`, behind everything the current stream has
        enqueued; the next step's head backward waits for it (shared_T).  `version`: the ParamStore.version the copy belongs to."""
        P = self.P
        ET = self._bufs.get(("w.sharedT", P.d, P.Vpad, self.dt))  # (only once a head backward has built it)
        if not self.head_nt or self.dt != torch.bfloat16 or ET is None or self._head8():
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            side.wait_event(ev)
            with ops.pinned_stream():
                ops.transpose_bf16(P.w("shared"), ET, P.Vpad, P.d)
            done = torch.cuda.Event()
            done.record(side)
        self._ET_version, self._ET_event = version, done

    # ------------------------------------------------------------------ full passes
    def forward_logits(self, pixels, ids, pos_ids, key_mask, B, T, *, save=False, seed=None, trunc_int32=False, stats=False, images=None):
        self._fp8_begin_pass()
        _, ehs = self.vit_forward(pixels, save, trunc_int32)
        hf = self.decoder_forward(ids, pos_ids, key_mask, ehs, B, T, save, seed, images=images)
        if stats:
            logits, stat = self.head_logits(hf, B * T, stats=True, fp8=True)
            return logits, ehs, stat
        return self.head_logits(hf, B * T, fp8=True), ehs

    def compact_head(self, hf, M: int, rows, packed: bool = False):
        """LM head on the loss-relevant rows only: gather hf[idx] -> [Mc, d] (zero pad to a multiple of 64 rows) and
        project.  Exact: loss_fn multiplies every other position by 0 (main.py:678).  packed: hf already holds exactly those
        rows, in that order (the decoder ran on them only): no gather."""
        P = self.P
        idx, Mc = rows
        Mcp = _rup(Mc, 64)
        if packed:
            hfc = hf
        else:
            hfc = self.buf("d.hfc", M, P.d)
            ops.copy_rows(hf, hfc, Mc, P.d, src_idx=idx)
        if Mcp > Mc:
            ops.zero(hfc[Mc:Mcp])
        logits = self.buf("d.logits", M, P.Vpad)
        stat = self.head_stats("d.logits", M)
        self._head_project(hfc, logits, Mc, stat)
        if Mcp > Mc:
            ops.zero(logits[Mc:Mcp])  # reduction padding of the dE GEMM (rows of an earlier, longer batch may linger here)
        return logits, stat

    def loss_only(self, pixels, ids, pos_ids, key_mask, labels, B, T, *, label_smoothing=0.0, rows=None, row_labels=None, pack=None,
                  images=None, row_weights=None):
        """eval_step's forward + loss (main.py:710-716).  images, row_weights: see loss_and_grads."""
        M = B * T
        pack = self._check_pack(pack, rows, T)
        self._check_images(pixels, B, images, pack)
        self._check_row_weights(row_weights, M if rows is None else rows[1])
        if rows is None:
            logits, _, stat = self.forward_logits(pixels, ids, pos_ids, key_mask, B, T, save=False, seed=None, stats=True, images=images)
            return self.loss_and_dlogits(logits, labels, key_mask.reshape(-1), M, label_smoothing, backward=False, stat=stat,
                                         row_weights=row_weights)
        self._fp8_begin_pass()
        _, ehs = self.vit_forward(pixels, False)
        hf = self.decoder_forward(ids, pos_ids, key_mask, ehs, B, T, False, None, pack=pack, images=images)
        logits, stat = self.compact_head(hf, M, rows, packed=pack is not None)
        return self.loss_and_dlogits(logits, row_labels, self.ones_i32(rows[1]), rows[1], label_smoothing, backward=False, stat=stat,
                                     row_weights=row_weights)

    # ------------------------------------------------------------------ teacher-forced scores (model.score)
    SCORE_CHUNK_ROWS = 4096  # materialised scoring head: rows per chunk — its logits never exceed loss_only's buffer for that many rows

    def score_head_free(self, Mc: int) -> bool:
        """does the scoring head of `Mc` rows run without logits?  bf16 storage with softmax partials, the planner gives the pick launch
        (ops.gemm pick_col / pick_out, out=None) to gemm_d2_kernel<2>, and MIC_SCORE_HEAD (read here, at call time) does not say
        `materialised` (A/B runs and tests)."""
        if self.dt != torch.bfloat16 or not self.use_head_stats or os.environ.get("MIC_SCORE_HEAD", "") == "materialised":
            return False
        plan = ops.gemm_plan([(Mc, self.P.Vpad, self.P.d)], kernel=True, pick=True)
        return plan["family"] == 6 and plan["epi"] == 2

    def score_rows(self, pixels, ids, pos_ids, key_mask, labels, B, T, *, seg, rows=None, row_labels=None, pack=None, images=None):
        """loss_only's forward (eval mode, no dropout; rows / pack / images as there) with a scorer's tail: returns
        (token_logprob fp32 [Mc] = -row_loss = log p(label | prefix, image) of the head's rows — the `rows` positions, or all B*T —,
        sums fp32 [n_seg]).  seg = (seg_off int32 [n_seg], seg_len int32 [n_seg]): sums[s] = the sum of token_logprob over head rows
        [seg_off[s], seg_off[s] + seg_len[s]) (mic_segment_sums: a caption's valid positions are consecutive head rows).
        Head: logits-free where `score_head_free` says so — the GEMM leaves softmax partials and each row's label logit, no
        `d.logits` buffer is touched or allocated (mic_ce_rows_picked) —, else materialised in chunks of SCORE_CHUNK_ROWS rows
        (mic_ce_rows_tiles / mic_ce_rows with label_smoothing 0).  Both forms give the same bits in bf16 storage."""
        P = self.P
        M = B * T
        pack = self._check_pack(pack, rows, T)
        self._check_images(pixels, B, images, pack)
        if self.fp8:
            raise ValueError("score_rows: scoring with fp8 GEMMs is not supported")
        _, ehs = self.vit_forward(pixels, False)
        hf = self.decoder_forward(ids, pos_ids, key_mask, ehs, B, T, False, None, pack=pack, images=images)
        Mc, lab = M, labels
        if rows is not None:
            idx, Mc = rows
            lab = row_labels
            if pack is None:  # (packed: hf already holds exactly those rows, in that order)
                hfc = self.buf("d.hfc", M, P.d)
                ops.copy_rows(hf, hfc, Mc, P.d, src_idx=idx)
                hf = hfc
        lse, rl = self.vec("ce.lse", _rup(M, ROWPAD)), self.vec("ce.rowloss", _rup(M, ROWPAD))
        if self.score_head_free(Mc):
            stat = self.buf("d.score.stat", M, 2 * (P.Vpad // 64), torch.float32)
            pick = self.vec("d.score.pick", _rup(M, ROWPAD))
            ops.gemm(hf, P.w("shared"), None, Mc, P.Vpad, P.d, bias=P.f32("flb"), rowstat=stat, rowstat_nvalid=P.V, pick_col=lab, pick_out=pick)
            ops.ce_rows_picked(P.V, stat, pick, lse, rl, Mc)
        else:
            cap = min(M, self.SCORE_CHUNK_ROWS)
            logits = self.buf("d.logits", cap, P.Vpad)
            stat = self.head_stats("d.logits", cap)
            for r0 in range(0, Mc, cap):
                n = min(cap, Mc - r0)
                self._head_project(hf[r0:], logits, n, stat, fp8=False)
                if stat is not None:
                    ops.ce_rows_tiles(logits, logits.stride(0), P.V, stat, lab[r0:], lse[r0:], rl[r0:], n)
                else:
                    ops.ce_rows(logits, logits.stride(0), P.V, lab[r0:], self.ones_i32(n), 0.0, lse[r0:], rl[r0:], n)
        seg_off, seg_len = seg
        n_seg = int(seg_off.numel())
        sums = self.vec("d.score.sums", n_seg)
        ops.segment_sums(seg_off, seg_len, rl, sums, n_seg, scale=-1.0)
        return rl[:Mc].neg(), sums

    def _check_images(self, pixels, B: int, images, pack):
        """the pass over B caption rows takes `images` distinct images (None: B): checked before anything is launched"""
        n = B if images is None else images
        if pixels.shape[0] != n:
            raise ValueError(f"pixels hold {pixels.shape[0]} images, the pass expects {n} (B={B}, images={images})")
        self._kv_group(B, images, pack)

    def _check_pack(self, pack, rows, T: int):
        """packed rows need the bf16-storage kernels (bf16 or fp8 GEMMs) and the compacted head on the same rows; any seq_len and any
        number of encoder positions (`packed_attn_tiled` picks the attention cores)"""
        if pack is None:
            return None
        if rows is None or rows[1] != pack[2]:
            raise ValueError("packed decoder rows go with the compacted LM head on the same rows (rows=(idx, n) with n == pack rows)")
        if self.dt != torch.bfloat16:
            raise ValueError("packed decoder rows: bfloat16 storage mode")
        return pack

    def ones_i32(self, n: int):
        """int32 ones [n] (the loss mask of the compacted rows): one buffer that only ever grows — the row count changes from step to
        step, a buffer per distinct count would accumulate"""
        t = self._bufs.get("ones_i32")
        if t is None or t.numel() < n:
            t = torch.ones(max(_rup(max(n, 1), 4096), 2 * (t.numel() if t is not None else 0)), dtype=torch.int32, device=self.dev)
            self._bufs["ones_i32"] = t
        return t[:n]

    def loss_and_grads(self, pixels, ids, pos_ids, key_mask, labels, B, T, *, label_smoothing=0.0, seed=None, rows=None,
                       row_labels=None, pack=None, images=None, row_weights=None):
        """value_and_grad(compute_loss) of train_step (main.py:688-697): grads land in ParamStore.grad.
        rows = (idx int32 [Mc] of the positions with loss mask 1, Mc) and row_labels = labels[idx] switch the LM head,
        the cross-entropy and their backward to those rows only (identical loss and gradients, ~(1 - Mc/M) less head work).
        images (None = B): the number of distinct images in `pixels` — G = B // images captions per image, caption row r belongs to
        image r // G.  The step is the one on pixels.repeat_interleave(G, 0): the image tower, the cross k/v projections and their
        backward run at images*S rows, an image's encoder states receive the sum of its captions' gradients.
        row_weights (None: the plain loss): fp32 device vector over the head's rows — the `rows` positions when the head is compacted,
        else all B*T — of per-row loss weights w: loss = sum w mask l / sum mask (the denominator does not depend on w; any finite
        value, zeros and negatives included), gradients those of that loss.  All weights 1.0 give the plain step's bits.  ValueError
        before any launch with fp8 GEMMs."""
        P = self.P
        self._check_images(pixels, B, images, None if pack is None else self._check_pack(pack, rows, T))
        self._check_row_weights(row_weights, B * T if rows is None else rows[1])
        P.ensure_grads()
        ops.zero(P.grad[P.atomic_begin:])
        M = B * T
        pack = self._check_pack(pack, rows, T)
        if rows is None:
            logits, ehs, stat = self.forward_logits(pixels, ids, pos_ids, key_mask, B, T, save=True, seed=seed, stats=True, images=images)
            loss = self.loss_and_dlogits(logits, labels, key_mask.reshape(-1), M, label_smoothing, backward=True, stat=stat,
                                         row_weights=row_weights)
        else:
            self._fp8_begin_pass()
            _, ehs = self.vit_forward(pixels, True)
            hf = self.decoder_forward(ids, pos_ids, key_mask, ehs, B, T, True, seed, pack=pack, images=images)
            logits, stat = self.compact_head(hf, M, rows, packed=pack is not None)
            loss = self.loss_and_dlogits(logits, row_labels, self.ones_i32(rows[1]), rows[1], label_smoothing, backward=True, stat=stat,
                                         row_weights=row_weights)
        dehs = self.decoder_backward(B, T, ids, pos_ids, key_mask, ehs, logits, seed, rows=rows, pack=pack, images=images)
        n_img = B if images is None else images
        if self.skip_vit_backward:
            self.vit_backward_bridge(n_img, dehs)
        else:
            self.vit_backward(n_img, dehs)
        self.dw_join()
        return loss
