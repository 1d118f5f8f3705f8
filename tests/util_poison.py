"""Scratch poisoning: no result may depend on what a buffer held before the call.

`Engine.buf` / `Engine.vec`, the fp8 operand state, the decode plans and the Trainer keep device tensors from call to call; a fresh
model holds zeros in all of them, so a forgotten zeroing or a reduction over the capacity instead of the valid rows passes every test
that builds its own model.  This module holds

  the inventory   `inventory(model, trainer)`: every device tensor that outlives a call, by name, with ONE contract out of CONTRACTS —
                  a table of name patterns without a catch-all: a tensor no pattern matches (or two match) raises, so a new buffer has
                  to be classified when it is added.  A contract may split a tensor into regions (`regions_of`).
      SCRATCH     fully written before it is read in every call: poisoned by `poison`.
      REST        holds a documented value between calls that the code relies on: never poisoned, asserted by `assert_rest` after every
                  call (padding rows behind a buffer's row capacity are zero at allocation and no kernel may write them: the fp32
                  weight-gradient GEMMs reduce over the 128-padded row count; unused fp8 scale slots are zero: the amax pass assumes it;
                  the deterministic-scatter workspace is owner = INT_MAX, count = 0, last = -1, multi_count = 0).
      STATE       carries meaning from call to call (weights, moments, the fp8 scale history, constants built once): left alone, the
                  reason stated in the table.
  the poison      NaN pass: fp32 / bf16 NaN, byte 0x7F for both fp8 formats.  Loud pass: +-3e38 (alternating) for fp32 / bf16, the
                  largest finite byte (+-, alternating) for fp8 — what a max, an amax or a comparison would swallow under NaN.  Integer
                  and byte buffers get 1 in both passes: a valid token id, row index, beam index, length and flag in every role listed
                  (INT_ROLES: read off the code per buffer) — never a pattern that could serve as an out-of-range index.  The one
                  exception is the fixed-point LayerNorm statistics of the decoder step (`g.lnstats`, int64 (sum, sum of squares), never
                  an index), which get (0, 2^40): a missing reset shows, and the variance read from it is huge, not negative.
  the comparison  `compare`: deterministic outputs bit for bit, atomically summed gradient leaves within 2e-4 x the leaf's maximum (the
                  summation-order bound of tests/test_model_gpu.py::test_packed_decoder_rows_change_nothing), and no NaN / Inf the
                  unpoisoned side does not hold.

The CPU companion (tests/test_poison_cpu.py) runs the patterns, the region logic, the table against a recorded name list and the
comparison against planted defects; tests/test_poison_gpu.py runs the matrix on the device."""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

SCRATCH, REST, STATE = "SCRATCH", "REST", "STATE"
NAN, LOUD = "nan", "loud"
PASSES = (NAN, LOUD)
LOUD_F32 = 3e38            # finite in fp32 and in bf16 (largest finite bf16: 3.39e38)
LOUD_BYTE = {torch.float8_e4m3fn: 0x7E, torch.float8_e5m2: 0x7B}   # largest finite magnitudes: 448 and 57344
NAN_BYTE = 0x7F            # NaN in e4m3fn (S.1111.111) and in e5m2 (S.11111.11)
INT_FILL = 1
LNSTATS_FILL = 1 << 40     # fixed-point (2^20) sums of the decoder step's LayerNorm statistics: data, never an index
ATOMIC_TOL = 2e-4          # x the leaf's maximum: the summation-order bound the project uses for atomically summed gradients
INT_MAX = 0x7FFFFFFF


class PoisonError(AssertionError):
    """a result depended on stale buffer contents, a REST region was left dirty, or a tensor has no contract"""


# ================================================================================================ the contract table
@dataclass(frozen=True)
class Rule:
    pattern: str              # fullmatch on the inventory name
    contract: str             # of the tensor, or of its live part when `split` names a region function
    reason: str               # one line: why this contract (STATE and REST: what the value means / who relies on it)
    split: Optional[str] = None      # region function in SPLITS
    int_role: Optional[str] = None   # integer / byte SCRATCH buffers: the role that makes the fill value 1 valid (INT_ROLES)
    live_in: Tuple[str, ...] = ()    # scenarios in which a SCRATCH tensor carries state and is left alone


# what the integer buffers hold and why 1 is in range there (the sizes below are those of every test configuration: vocabulary >= 1003,
# at least 2 decoder rows, max_length >= 2)
INT_ROLES = {
    "token": "a token id: 1 < vocabulary size",
    "row": "a decoder row index: 1 < rows (every scenario runs at least 2 rows)",
    "flag": "a 0 / 1 flag or counter word that the call resets before its first read",
    "key": "PRNG key words: any bit pattern is a key",
    "stats": "fixed-point (sum, sum of squares) pairs, never an index: (0, LNSTATS_FILL)",
}

# activation / gradient buffers of the training passes (Engine.buf(name, rows, cols)): the rows below the capacity `rows` are written
# before they are read in every pass, the rows between it and the 128-padded allocation are zero for ever
_V = r"v(\d+|_)"
_D = r"d(\d+|_)"
_PAD = "rows at and above the capacity are allocation zeros that no kernel writes: the fp32 weight-gradient GEMMs and the patch-embedding dW reduce over the 128-padded row count"
RULES: List[Rule] = [
    # ---- Engine._bufs: training / eval passes
    Rule(r"buf:v\.(patches|pe|emb|x0|ehs|pre\.stats)", SCRATCH, _PAD, "pad_rows"),
    Rule(rf"buf:{_V}\.(st1|st2|a1|a2|qkv|ctx|xm|z|u|xo\d?)", SCRATCH, _PAD, "pad_rows"),
    Rule(rf"vec:{_V}\.lse", SCRATCH, "written by the attention forward of the same pass"),
    Rule(r"buf:vb\.(dx|dz|da|dxm|dctx|dqkv|demb|dpe)(\.\d+)?", SCRATCH, _PAD, "pad_rows"),
    Rule(r"buf:lnp\.\w+\.\d+", SCRATCH, "LayerNorm gradient partials: blocks(rows) written, the same blocks reduced", "pad_rows"),
    Rule(r"buf:d\.(h0|x0|emb\.stats|hf|hfc|hfT|f\.stats|ckvcat|logits|logits\.stat|dlogitsT)", SCRATCH, _PAD, "pad_rows"),
    Rule(r"buf:d_\.ckvcat", SCRATCH, _PAD, "pad_rows"),
    Rule(rf"buf:{_D}\.(stats|a_sa|qkv|ctx|x1|a_ca|cq|ckv|cctx|x2|a_ff|z|u|x3\d?)", SCRATCH, _PAD, "pad_rows"),
    Rule(rf"vec:{_D}\.c?lse", SCRATCH, "written by the attention forward of the same pass"),
    Rule(r"buf:db\.(dhf|dhfc|dhf32|dx|dxm_[abc]|dz|da|dx2|dctx|dq|dkv|dkvcat|dx1|dqkv|dehs|dehs32|dh0)(\.\d+)?", SCRATCH, _PAD, "pad_rows"),
    Rule(r"vec:db\.ids_x", SCRATCH, "ids of the deferred embedding rows: rewritten up to the capacity by every backward", int_role="token"),
    Rule(r"vec:ce\.(lse|rowloss|loss|denom)", SCRATCH, "cross-entropy rows and the two scalars: plain stores by every pass"),
    Rule(r"buf:head\.dl\.q8", SCRATCH, _PAD, "pad_rows"),
    Rule(r"vec:head\.dl\.(state|coef)", SCRATCH, "closed-form scale and label coefficients of the fp8 CE backward: plain stores"),
    # ---- fp8 operand bytes (Engine.buf through Fp8State.quant / target)
    Rule(rf"buf:({_V}|{_D}|f8)\.(qkv|cq|ckv|fc1|fc2)\.x\.q8", SCRATCH, _PAD, "pad_rows"),
    Rule(r"buf:(d\.ehs\.ckv|d_?\.ckvcat)\.x\.q8", SCRATCH, _PAD, "pad_rows"),
    Rule(r"buf:f8\.(dec|vit)\.(qkv|cq|ckv|fc1|fc2)\.dy\.\d+\.q8", SCRATCH, _PAD, "pad_rows"),
    Rule(r"buf:f8\.ckvcat\.dy\.q8", SCRATCH, _PAD, "pad_rows"),
    Rule(r"buf:head\.x\.q8", SCRATCH, _PAD, "pad_rows"),
    # ---- Engine._bufs: the cached decoder step (generate / decode)
    Rule(r"buf:(s\d+\.)?g\.(h0|x|a|ctx|x1|x2|q|u|hf|logits|logits\.stat|logits\.sl|logits\.sl\.stat)", SCRATCH, _PAD, "pad_rows"),
    Rule(r"buf:(s\d+\.)?g\.lnstats", SCRATCH, "(sum, sum of squares) per row: zeroed at the top of every decoder step, then added to", "pad_rows",
         int_role="stats"),
    Rule(r"buf:(s\d+\.)?g\.(ehs|ckv\d+)", SCRATCH, "encoder states and cross K/V: projected once per generate call; across the steps of a "
         "decode() sequence they are the call's state", "pad_rows", live_in=("decode",)),
    # ---- Engine._bufs: STATE
    Rule(r"buf:w\.sharedT", STATE, "E^T, a derived weight copy (weight-coherence suite)"),
    Rule(r"buf:ones_i32", STATE, "int32 ones, built once and only ever grown: the loss mask of the compacted rows"),
    # ---- Fp8State
    Rule(r"f8\.w\.[\w.]+\.(q|qT)", STATE, "fp8 weight copies, derived from the weights (weight-coherence suite)"),
    Rule(r"f8\.w_state", STATE, "(amax, 1 / scale) per weight: the scale source of the next re-quantisation"),
    Rule(r"f8\.w_part", STATE, "partial maxima of the weights as last quantised: rolled into w_state by the next refresh"),
    Rule(r"f8\.a_state", STATE, "(amax, 1 / scale) per activation tag: the delayed-scaling history; slots not handed out yet are zero and "
         "the first amax pass over a new tag relies on it", "slots"),
    Rule(r"f8\.a_part", STATE, "partial maxima recorded by the last pass: rolled into a_state by the next begin_pass; unused slots zero", "slots"),
    # ---- LayerNorm folds, shortlists
    Rule(r"lnf\.[\w.]+\.(w|colsum|bias)", STATE, "LayerNorm-folded decoder-step weights, derived from the weights (weight-coherence suite)"),
    Rule(r"shortlist\.(E|bias)", STATE, "gathered rows / bias entries of the tied embedding, derived from the weights; the padding rows and "
         "entries behind the Ns valid ones are zero at allocation, never written, and the head GEMM runs over them", "shortlist_pad"),
    Rule(r"shortlist\.(map|rows)", STATE, "the sorted token ids of the list, uploaded once"),
    # ---- ParamStore
    Rule(r"store\.(master|lp)", STATE, "the weights and their compute-dtype copy"),
    Rule(r"store\.(m|v)", STATE, "AdamW moments"),
    Rule(r"store\.acc", STATE, "gradient sum of the micro-steps taken so far"),
    Rule(r"store\.grad", SCRATCH, "segments below atomic_begin are overwritten by backward, the atomic region is zeroed at the top of every "
         "pass; with a frozen image tower its segments keep what they held and nothing reads them"),
    # ---- Trainer
    Rule(r"trainer\.hyper", STATE, "(lr, count) of the pending optimizer step: written on micro-step 0, read on the last"),
    Rule(r"trainer\.loss_sum", STATE, "sum of the micro-step losses of the pending optimizer step"),
    Rule(r"trainer\.metrics_buf", SCRATCH, "both entries written by eval_step / the multi-rank train_step before they are read"),
    Rule(r"trainer\.row_flag", SCRATCH, "cleared and set by mic_row_flags at the top of every optimizer step", int_role="flag"),
    Rule(r"trainer\.clip_(partials|out)", SCRATCH, "every slot / both values stored by each clipped step before they are read"),
    Rule(r"trainer\.pos\.\d+x\d+", STATE, "position ids 0 .. T-1 per batch shape, built once"),
    Rule(r"trainer\.groups", STATE, "the run table of the grouped AdamW, uploaded once"),
    Rule(r"trainer\.det_ws", REST, "workspace of mic_embed_rows_add_det: owner = INT_MAX, count = 0, last = -1, multi_count = 0 between "
         "calls (the kernels restore it); the multi list behind them is scratch (source row indices, read up to the count the call "
         "itself wrote)", "det_ws", int_role="row"),
    Rule(r"reducer\.(stage\.\d+|emu_scratch)", SCRATCH, "staging copy of one bucket: written by the narrowing copy before the collective reads it"),
    # ---- decode plans
    Rule(r"plan\.\w+\.(sub\.)?(pos_all|score0|rows)", STATE, "constants of the plan (position ids, the initial beam scores, the identity row map): built once"),
    Rule(r"plan\.\w+\.(sub\.)?(sequences|running_seq|seq|next_token|start_rows|bos_rows|top_idx|cand_idx|drawn)", SCRATCH,
         "token ids: reset or fully written by every call before the first read", int_role="token"),
    Rule(r"plan\.\w+\.(sub\.)?src_row", SCRATCH, "beam ancestry (row indices): zeroed and column 0 set by every call", int_role="row"),
    Rule(r"plan\.\w+\.(sub\.)?(finished|flags|gstate|lim)", SCRATCH, "flags, counters and tie limits: reset by every call / written by the "
         "step before they are read", int_role="flag"),
    Rule(r"plan\.\w+\.(sub\.)?keys", SCRATCH, "per-step PRNG keys: the whole table is copied in by every call", int_role="key"),
    Rule(r"plan\.\w+\.(sub\.)?(top_val|cand_val|scores|running_scores|thr)", SCRATCH, "scores and thresholds: reset by every call / written by "
         "the step before they are read"),
    Rule(r"plan\.\w+\.(sub\.)?[kv]\d+", SCRATCH, "self-attention cache: a step reads only the slots <= its own index, all written earlier in the same call"),
]
_COMPILED = [(re.compile(r.pattern), r) for r in RULES]


def classify(name: str) -> Rule:
    """the one rule whose pattern matches `name`; none or several: PoisonError"""
    hits = [r for c, r in _COMPILED if c.fullmatch(name)]
    if len(hits) != 1:
        raise PoisonError(f"inventory: {name!r} has {len(hits)} contracts ({[h.pattern for h in hits]}): every tensor that outlives a call needs "
                          "exactly one row in tests/util_poison.py RULES")
    return hits[0]


# ================================================================================================ regions
@dataclass(frozen=True)
class Region:
    contract: str
    index: tuple               # t[index] is the region (row slices: contiguous)
    rest: Optional[int] = None  # REST: the value every element holds between calls


def _rows(a, b=None):
    return (slice(a, b),)


def _split_pad_rows(shape, rule, meta):
    """[0, rows) under the rule's contract, [rows, allocation) REST zero; `rows` = the capacity the buffer was asked for"""
    rows = int(meta.get("rows", shape[0]))
    rows = max(0, min(rows, shape[0]))
    out = [Region(rule.contract, _rows(0, rows))] if rows > 0 else []
    if rows < shape[0]:
        out.append(Region(REST, _rows(rows, None), 0))
    return out


def _split_slots(shape, rule, meta):
    """fp8 slot tables: the first `slots` rows carry the history, the others have never been handed out and are zero"""
    n = max(0, min(int(meta.get("slots", shape[0])), shape[0]))
    out = [Region(rule.contract, _rows(0, n))] if n > 0 else []
    if n < shape[0]:
        out.append(Region(REST, _rows(n, None), 0))
    return out


def _split_shortlist_pad(shape, rule, meta):
    n = max(0, min(int(meta["Ns"]), shape[0]))
    out = [Region(rule.contract, _rows(0, n))]
    if n < shape[0]:
        out.append(Region(REST, _rows(n, None), 0))
    return out


def _split_det_ws(shape, rule, meta):
    V = int(meta["vocab"])
    return [Region(REST, _rows(0, V), INT_MAX), Region(REST, _rows(V, 2 * V), 0), Region(REST, _rows(2 * V, 3 * V), -1),
            Region(REST, _rows(3 * V, 3 * V + 1), 0), Region(SCRATCH, _rows(3 * V + 1, None))]


SPLITS: Dict[str, Callable] = {"pad_rows": _split_pad_rows, "slots": _split_slots, "shortlist_pad": _split_shortlist_pad, "det_ws": _split_det_ws}


def regions_of(shape, rule: Rule, meta: dict) -> List[Region]:
    """the regions of a tensor of `shape` under `rule`: disjoint, covering every row"""
    if rule.split is None:
        return [Region(rule.contract, (slice(None),), 0 if rule.contract == REST else None)]
    return SPLITS[rule.split](tuple(shape), rule, meta)


# ================================================================================================ the inventory walk
@dataclass
class Entry:
    name: str
    tensor: torch.Tensor
    rule: Rule
    meta: dict = field(default_factory=dict)

    @property
    def regions(self) -> List[Region]:
        return regions_of(self.tensor.shape, self.rule, self.meta)


def walk(model, trainer=None):
    """(name, tensor, meta) of every device tensor that outlives a call.  Views into a listed tensor (parameter segments, scale slots,
    the fp8 inputs kept for backward) are not listed again."""
    eng, st = model.engine, model.store
    for key, t in eng._bufs.items():
        if isinstance(key, tuple) and len(key) == 4:
            yield f"buf:{key[0]}", t, {"rows": key[1]}
        elif isinstance(key, tuple):
            yield f"vec:{key[0]}", t, {}
        else:
            yield f"buf:{key}", t, {}
    f8 = getattr(eng, "f8", None)
    if f8 is not None:
        for n, w in f8.weights.items():
            yield f"f8.w.{n}.q", w.q, {}
            yield f"f8.w.{n}.qT", w.qT, {}
        yield "f8.w_state", f8.w_state, {}
        yield "f8.a_state", f8.a_state, {"slots": len(f8.slots)}
        if f8.w_part is not None:
            yield "f8.w_part", f8.w_part, {}
            yield "f8.a_part", f8.a_part, {"slots": len(f8.slots)}
    for wn, (w, cs, b) in eng._lnf.items():
        yield f"lnf.{wn}.w", w, {}
        yield f"lnf.{wn}.colsum", cs, {}
        yield f"lnf.{wn}.bias", b, {}
    plans = model.__dict__.get("_decode_plans", {})
    lists = {id(s): s for s in model.__dict__.get("_shortlists", {}).values()}
    lists.update({id(p.shortlist): p.shortlist for p in plans.values() if p.shortlist is not None})
    for sl in lists.values():
        yield "shortlist.E", sl.E, {"Ns": sl.Ns}
        yield "shortlist.bias", sl.bias, {"Ns": sl.Ns}
        yield "shortlist.map", sl.map, {}
        yield "shortlist.rows", sl._rows, {}
    for k in ("master", "lp", "grad", "acc", "m", "v"):
        t = getattr(st, k)
        if t is not None and not (k == "lp" and t is st.master):
            yield f"store.{k}", t, {}
    if trainer is not None:
        tr = trainer
        for k in ("hyper", "metrics_buf", "_row_flag", "_clip_partials", "_clip_out", "_loss_sum"):
            t = getattr(tr, k, None)
            if t is not None:
                yield "trainer." + k.lstrip("_"), t, {}
        for (B, T), t in tr._pos.items():
            yield f"trainer.pos.{B}x{T}", t, {}
        if tr._groups is not None:
            yield "trainer.groups", tr._groups.dev, {}
        if tr._det_ws is not None:
            yield "trainer.det_ws", tr._det_ws, {"vocab": st.g("shared").numel() // st.d}
        r = tr.reducer
        for i, t in enumerate(r.stage or ()):
            yield f"reducer.stage.{i}", t, {}
        if getattr(r, "_emu_scratch", None) is not None:
            yield "reducer.emu_scratch", r._emu_scratch, {}
    for key, plan in plans.items():
        for n, t in plan.t.items():
            yield f"plan.{key[0]}.{n}", t, {}
        for sub in plan.subs:
            for n, t in sub.t.items():
                yield f"plan.{key[0]}.sub.{n}", t, {}


def inventory(model, trainer=None) -> List[Entry]:
    """every tensor of `walk` with its contract; a tensor without exactly one raises PoisonError"""
    return [Entry(name, t, classify(name), meta) for name, t, meta in walk(model, trainer)]


def names(model, trainer=None) -> List[str]:
    return sorted({name for name, _, _ in walk(model, trainer)})


# ================================================================================================ the poison
def _flat(t: torch.Tensor) -> torch.Tensor:
    if not t.is_contiguous():
        raise PoisonError("poison: a region must be contiguous")
    return t.view(-1)


def poison_(t: torch.Tensor, how: str, int_fill: int = INT_FILL) -> None:
    """fill the contiguous tensor (or row slice) `t` in place with the pattern of pass `how` for its dtype"""
    if t.numel() == 0:
        return
    if not t.is_contiguous():  # (a column range of a cache): the pattern through a contiguous temporary
        tmp = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        poison_(tmp, how, int_fill)
        t.copy_(tmp)
        return
    f = _flat(t)
    if t.dtype in LOUD_BYTE:
        b = f.view(torch.uint8)
        if how == NAN:
            b.fill_(NAN_BYTE)
        else:
            b.fill_(LOUD_BYTE[t.dtype])
            b[1::2] |= 0x80
    elif t.dtype.is_floating_point:
        if how == NAN:
            f.fill_(float("nan"))
        else:
            f.fill_(LOUD_F32)
            f[1::2] = -LOUD_F32
    elif t.dtype == torch.bool:
        f.fill_(True)
    elif int_fill == "stats":  # [..][2] = (sum, sum of squares): (0, LNSTATS_FILL) — a huge variance, so whatever reads it stays finite
        f.fill_(0)
        f[1::2] = LNSTATS_FILL
    else:
        f.fill_(int_fill)


def _int_fill(entry: Entry):
    """the fill value of an integer / byte SCRATCH tensor, None where the table names no role that makes one safe"""
    if entry.rule.int_role is None:
        return None
    return "stats" if entry.rule.int_role == "stats" else INT_FILL


def poison(entries: List[Entry], how: str, scenario: str = "", sync=None) -> Dict[str, str]:
    """poison every SCRATCH tensor / region of `entries` (device idle before and after: `sync`); returns {name: reason} of the SCRATCH
    tensors left alone (integer buffers without a safe value, tensors that carry state in this scenario)"""
    assert how in PASSES, how
    if sync is not None:
        sync()
    skipped = {}
    for e in entries:
        if scenario in e.rule.live_in:
            if e.rule.contract == SCRATCH:
                skipped[e.name] = f"carries state in scenario {scenario!r}"
            continue
        isint = not (e.tensor.dtype.is_floating_point or e.tensor.dtype in LOUD_BYTE)
        fill = INT_FILL
        if isint:
            fill = _int_fill(e)
        for rg in e.regions:
            if rg.contract != SCRATCH:
                continue
            if isint and fill is None:
                skipped[e.name] = "integer buffer without a stated role: no value is known to be safe"
                continue
            poison_(e.tensor[rg.index], how, fill)
    if sync is not None:
        sync()
    return skipped


def rest_violations(entries: List[Entry]) -> List[str]:
    out = []
    for e in entries:
        for rg in e.regions:
            if rg.contract != REST:
                continue
            v = e.tensor[rg.index]
            if v.numel() == 0:
                continue
            bad = (v.view(torch.uint8) if v.dtype in LOUD_BYTE else v) != rg.rest  # (fp8 regions rest at byte 0)
            n = int(bad.sum())
            if n:
                out.append(f"{e.name}{list(e.tensor.shape)} rows {rg.index[0].start}:{rg.index[0].stop}: {n} of {v.numel()} elements are not the rest "
                           f"value {rg.rest}")
    return out


def assert_rest(entries: List[Entry], what: str = "") -> None:
    """every REST region holds its rest value (the device must be idle)"""
    bad = rest_violations(entries)
    if bad:
        raise PoisonError(f"{what}: REST regions left dirty: " + "; ".join(bad[:6]) + (f" (+{len(bad) - 6} more)" if len(bad) > 6 else ""))


def state_entries(entries: List[Entry]) -> Dict[str, Entry]:
    return {e.name: e for e in entries if e.rule.contract == STATE}


def copy_state(src: List[Entry], dst: List[Entry]) -> None:
    """dst's STATE tensors := src's (the twins share one call history; this removes the summation-order noise of the atomically summed
    gradients from what the two carry into the measured call)"""
    a, b = state_entries(src), state_entries(dst)
    assert set(a) == set(b), sorted(set(a) ^ set(b))
    for k, e in a.items():
        assert b[k].tensor.shape == e.tensor.shape and b[k].tensor.dtype == e.tensor.dtype, k
        b[k].tensor.copy_(e.tensor)


# ================================================================================================ the comparison core
def _bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().contiguous()
    if t.dtype in LOUD_BYTE:
        return t.view(torch.uint8)
    if t.dtype.is_floating_point:
        return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _nonfinite(t: torch.Tensor) -> torch.Tensor:
    if t.dtype in LOUD_BYTE:
        t = t.float()
    return ~torch.isfinite(t) if t.dtype.is_floating_point else torch.zeros(t.shape, dtype=torch.bool)


def compare(got: Dict[str, torch.Tensor], want: Dict[str, torch.Tensor], atomic=(), what: str = "") -> None:
    """`got` (the poisoned side) against `want` (the unpoisoned twin or a fresh model), host tensors by name: bit for bit, except the
    names in `atomic` (|got - want| <= ATOMIC_TOL x max |want|); and nowhere a NaN / Inf that `want` does not hold at that element"""
    if set(got) != set(want):
        raise PoisonError(f"{what}: outputs differ in kind: {sorted(set(got) ^ set(want))}")
    atomic = set(atomic)
    for k in sorted(want):
        g, w = torch.as_tensor(got[k]).cpu(), torch.as_tensor(want[k]).cpu()
        if g.shape != w.shape or g.dtype != w.dtype:
            raise PoisonError(f"{what}: {k}: {tuple(g.shape)} {g.dtype} against {tuple(w.shape)} {w.dtype}")
        new = _nonfinite(g) & ~_nonfinite(w)
        if new.any():
            raise PoisonError(f"{what}: {k}: {int(new.sum())} of {g.numel()} elements are NaN / Inf where the unpoisoned side is finite")
        if k in atomic:
            gf, wf = g.double(), w.double()
            fin = torch.isfinite(wf)
            sc = float(wf[fin].abs().max()) if fin.any() else 0.0
            err = float((gf - wf)[fin].abs().max()) if fin.any() else 0.0
            if err > ATOMIC_TOL * max(sc, 1e-12):
                raise PoisonError(f"{what}: {k}: |diff| {err:.3e} > {ATOMIC_TOL} x max {sc:.3e} (atomically summed leaf)")
            continue
        bad = _bits(g) != _bits(w)
        if bad.any():
            i = tuple(int(x) for x in bad.nonzero()[0])
            raise PoisonError(f"{what}: {k}: {int(bad.sum())} of {g.numel()} elements differ bit for bit, first at {i}: "
                              f"{g[i].item() if g.dim() else g.item()!r} != {w[i].item() if w.dim() else w.item()!r}")


# ================================================================================================ device-side helpers of the GPU suite
def sync():
    torch.cuda.synchronize()


def grad_outputs(store, skip=()) -> Tuple[Dict[str, torch.Tensor], set]:
    """({"grad:<segment>": host copy}, names of the atomically summed ones).  Atomically summed: every segment of the trailing atomic
    region (ParamStore.atomic_begin), and the two in front of it that also receive fp32 atomics — `shared` (the input-embedding rows
    of mic_embed_bwd and the label terms of the fp8 head land on top of the dense head gradient) and `flb` (row sums out of the dE GEMM /
    column sums out of the CE backward)."""
    flat = store.grad.detach().cpu()
    out, atomic = {}, set()
    for name, s in store.segs.items():
        if name in skip:
            continue
        out["grad:" + name] = flat[s.offset: s.offset + s.numel].clone()
        if s.offset >= store.atomic_begin or name in ("shared", "flb"):
            atomic.add("grad:" + name)
    return out, atomic


# ================================================================================================ scenarios: engine passes
B_, T_ = 6, 16
NEAR_FULL = [16, 15, 15, 15, 15, 15]  # captions that fill nearly every row: 91 loss rows, so the compacted head still has padding rows
DROP_SEED = 4242
GROUPS = [dict(match=r"vit.*|patch\.w", frozen=True), dict(match=r"dec\d+\..*", lr_scale=0.5)]

# mode -> storage dtype, LM head on the loss rows only, packed decoder rows, fp8 scaling, MIC_FP8_HEAD
ENGINE_MODES = {
    "fp32-padded": dict(dtype=torch.float32, compact=False, packed=False),
    "fp32-compact": dict(dtype=torch.float32, compact=True, packed=False),
    "bf16-padded": dict(dtype=torch.bfloat16, compact=False, packed=False),
    "bf16-compact": dict(dtype=torch.bfloat16, compact=True, packed=False),
    "bf16-packed": dict(dtype=torch.bfloat16, compact=True, packed=True),
    "fp8delayed-all": dict(dtype=torch.bfloat16, compact=True, packed=True, scaling="delayed", head="all"),
    "fp8delayed-0": dict(dtype=torch.bfloat16, compact=True, packed=True, scaling="delayed", head="0"),
    "fp8current-all": dict(dtype=torch.bfloat16, compact=True, packed=True, scaling="current", head="all"),
    "fp8current-0": dict(dtype=torch.bfloat16, compact=True, packed=True, scaling="current", head="0"),
}


def engine_model(mode: str, dev, **over):
    """(oracle config, product model) of an engine-pass mode: the small configuration, dropout on (the config's 0.1)"""
    import os

    from util_small import make_pair

    md = ENGINE_MODES[mode]
    rc, _, model = make_pair(md["dtype"], dev, gelu="tanh", decoder_ln_eps=1e-6, **over)
    if "scaling" in md:
        assert os.environ.get("MIC_FP8_HEAD") == md["head"], "the caller sets MIC_FP8_HEAD (monkeypatch) before the model is built"
        model.engine.set_gemm_dtype("fp8", scaling=md["scaling"])
        assert model.engine.fp8_head == {"all": 2, "0": 0}[md["head"]]
    return rc, model


def caption_batch(rc, B: int, T: int, seed: int, lens=None):
    """util_small.batch, or — lens given — captions of exactly those lengths (labels of `lens[b]` tokens, the last one EOS)"""
    from util_small import batch

    if lens is None:
        return batch(rc, B, T, seed=seed)
    if lens == "full":
        return batch(rc, B, T, seed=seed, ragged=False)
    assert len(lens) == B
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(B, rc.image_size, rc.image_size, 3, generator=g).clamp(-1.8, 2.2)
    labels = torch.full((B, T), rc.pad_token_id, dtype=torch.int64)
    mask = torch.zeros((B, T), dtype=torch.int64)
    for b, n in enumerate(lens):
        labels[b, :n] = torch.randint(4, rc.vocab_size - 20, (n,), generator=g)
        labels[b, n - 1] = rc.eos_token_id
        mask[b, :n] = 1
    dec_in = torch.full_like(labels, rc.pad_token_id)
    dec_in[:, 1:] = labels[:, :-1]
    return px, labels, mask, dec_in


def engine_pass(model, rc, mode: str, bt, ls: float, train: bool, T: int = T_) -> Tuple[Dict[str, torch.Tensor], set]:
    """one `loss_and_grads` (train, dropout seed DROP_SEED) or `loss_only` call on the host batch `bt`; returns (outputs, atomic names):
    the loss, the head's rows of the logits buffer (after a training pass: whatever the backward left there — dlogits in place, or
    the logits beside the fp8 head) and, after a training pass, every gradient segment"""
    from mic_amd import loss_rows, packed_rows

    md = ENGINE_MODES[mode]
    eng, st, d = model.engine, model.store, model._dev
    px, labels, mask, dec_in = bt
    B = px.shape[0]
    kw, n_head = {}, B * T
    if md["compact"]:
        idx, rl = loss_rows(mask.numpy(), labels.numpy())
        assert 0 < len(idx) < B * T and len(idx) % 64 != 0, "the compacted head needs padding rows for this to test anything"
        kw, n_head = dict(rows=(d(idx, torch.int32), len(idx)), row_labels=d(rl, torch.int32)), len(idx)
    if md["packed"]:
        q_off, q_len, ids, pos = (d(t, torch.int32) for t in packed_rows(mask.numpy(), dec_in.numpy()))
        kw["pack"], key_mask = (q_off, q_len, n_head), None
    else:
        ids = d(dec_in, torch.int32).reshape(-1)
        pos = torch.arange(T, dtype=torch.int32, device=model.device)[None].expand(B, T).contiguous().reshape(-1)
        key_mask = d(mask, torch.int32)
    args = (d(px, torch.float32), ids, pos, key_mask, d(labels, torch.int32).reshape(-1), B, T)
    if train:
        loss = eng.loss_and_grads(*args, label_smoothing=ls, seed=DROP_SEED, **kw)
    else:
        loss = eng.loss_only(*args, label_smoothing=ls, **kw)
    sync()
    out = {"loss": loss.detach().reshape(1).cpu(), "logits": eng.buf("d.logits", B * T, st.Vpad)[:n_head, : st.V].detach().cpu()}
    atomic = set()
    if train:
        g, atomic = grad_outputs(st)
        out.update(g)
        if eng.defer_embed:
            # the sparse rows of the tied embedding as the data-parallel step hands them on (ids, dh0 rows, count): the ids, and what
            # their consumer — the deterministic scatter — makes of them (rows with id -1 are skipped, whatever they hold)
            from mic_amd import ops

            ids_x, dh0, n = eng.embed_rows
            out["embed_rows.ids"] = ids_x[:n].detach().cpu()
            rows = st.g("shared").numel() // st.d
            table = torch.zeros(rows, st.d, dtype=torch.float32, device=model.device)
            ops.embed_rows_add_det(ids_x, dh0, eng.embed_scale, table, n, st.d, ops.embed_rows_add_det_workspace(rows, model.device))
            sync()
            out["embed_rows.table"] = table.cpu()
    return out, atomic


def refused_engine_call(model, rc, bt, T: int = T_):
    """a call a host check refuses (packed rows without the compacted head) — after the pass's first device work has been queued"""
    from mic_amd import packed_rows

    d = model._dev
    px, labels, mask, dec_in = bt
    q_off, q_len, ids, pos = (d(t, torch.int32) for t in packed_rows(mask.numpy(), dec_in.numpy()))
    try:
        model.engine.loss_and_grads(d(px, torch.float32), ids, pos, None, d(labels, torch.int32).reshape(-1), px.shape[0], T,
                                    pack=(q_off, q_len, int(q_len.sum())))
    except ValueError:
        sync()
        return
    raise AssertionError("packed rows without rows= were not refused")


# ================================================================================================ scenarios: Trainer
TRAINER_CASES = {
    "overlap": dict(bucket_mb=0.25),
    "one_launch": dict(overlap_optimizer=False),
    "accumulate": dict(accumulate_steps=2, bucket_mb=0.25),
    "clip": dict(max_grad_norm=1.0, bucket_mb=0.25),
    "groups": dict(param_groups=GROUPS, bucket_mb=0.25),
}


def batch_dict(bt):
    px, labels, mask, dec_in = bt
    return {"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}


def trainer_pair(case: str, dtype, dev):
    from mic_amd import Trainer, create_learning_rate_fn
    from util_small import make_pair

    rc, _, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6)
    tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 2, 2e-3), weight_decay=0.01, label_smoothing_factor=0.1, seed=42, **TRAINER_CASES[case])
    return rc, model, tr


def frozen_segments(tr) -> set:
    """segments a param_groups Trainer freezes (their gradients keep what they held when backward stops at the bridge)"""
    if tr._group_runs is None:
        return set()
    st = tr.model.store
    out = set()
    for name, s in st.segs.items():
        if any(f and b <= s.offset and s.offset + s.numel <= e for (b, e, _, _, f) in tr._group_runs):
            out.add(name)
    return out


def trainer_outputs(tr, metrics, with_grads: bool) -> Tuple[Dict[str, torch.Tensor], set]:
    """what a step returned and left behind: its metrics, the weights per segment and — after a training micro-step — the gradients.
    Atomic (summation-order bound): the atomically summed gradient leaves, grad_norm (a sum over them) and, once an optimizer step has
    consumed such gradients, nothing of the weights — those segments are held to the NaN / Inf rule alone (`loose`)."""
    st = tr.model.store
    sync()
    out = {"metric:" + k: torch.as_tensor(v).detach().reshape(1).float().cpu() for k, v in metrics.items()}
    atomic = {"metric:grad_norm"} & set(out)
    if with_grads:
        g, ga = grad_outputs(st, skip=frozen_segments(tr))
        out.update(g)
        atomic |= ga
    flat = st.master.detach().cpu()
    for name, s in st.segs.items():
        out["w:" + name] = flat[s.offset: s.offset + s.numel].clone()
    return out, atomic


def loosen_weights(got, want, tr, clipped: bool):
    """weights that an optimizer step moved by atomically summed gradients (or, under clipping, by a norm over them) cannot be held
    bit for bit: only the NaN / Inf rule applies to them — the comparison sees them as finite-or-not"""
    st = tr.model.store
    for name, s in st.segs.items():
        if clipped or s.offset >= st.atomic_begin or name in ("shared", "flb"):
            for side in (got, want):
                side["w:" + name] = torch.isfinite(side["w:" + name])


# ================================================================================================ scenarios: inference
ALLOWED = np.array([2] + list(range(20, 60)), dtype=np.int32)  # EOS = forced EOS = 2 and 40 ordinary ids
GEN_LEN = 8
GENERATE_CASES = {
    "greedy": dict(max_length=GEN_LEN, num_beams=1),
    "sample": dict(max_length=GEN_LEN, num_beams=1, do_sample=True, prng_key=7),
    "beam4": dict(max_length=GEN_LEN, num_beams=4),
    "languages": dict(max_length=GEN_LEN, num_beams=4, forced_bos_token_id=[996, 995]),
    "nreturn3": dict(max_length=GEN_LEN, num_beams=4, num_return_sequences=3),
    "sample-nreturn3": dict(max_length=GEN_LEN, num_beams=1, do_sample=True, prng_key=7, num_return_sequences=3),
    "shortlist": dict(max_length=GEN_LEN, num_beams=4, allowed_token_ids=ALLOWED),
}


def set_eos_bias(model, rc, value: float):
    """final_logits_bias[EOS] := value through the params setter (the weights move: ParamStore.version advances)"""
    from mic_amd.params import flatten_tree, unflatten_tree

    flat = flatten_tree(model.params)
    flb = np.array(flat["final_logits_bias"], dtype=np.float32)
    flb[0, rc.eos_token_id] = value
    flat["final_logits_bias"] = flb
    model.params = unflatten_tree(flat)


def pixels(rc, B: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, rc.image_size, rc.image_size, 3, generator=g).clamp(-1.8, 2.2).numpy()


def generate_outputs(model, px, kw) -> Dict[str, torch.Tensor]:
    """sequences and scores of a generate call, and the logits of the last decoder step it issued as they lie in the engine's buffer.
    (The small random models repeat a token and their beam scores are multiples of -1e7 / length: the tokens and scores alone would
    not show a decoder step that computed something else; the last step's logits are a function of the whole chain — every cache
    slot, the cross K/V, the LayerNorm statistics.)"""
    o = model.generate(px, **kw)
    sync()
    out = {"sequences": o.sequences.detach().cpu()}
    if o.get("scores") is not None:
        out["scores"] = o.scores.detach().cpu()
    for key, t in model.engine._bufs.items():
        if isinstance(key, tuple) and key[0] in ("g.logits", "g.logits.sl"):
            out[f"last step {key[0]}[{key[1]}]"] = t[: key[1]].detach().cpu()
    return out


def poison_user_cache(cache: dict, how: str):
    """positions > cache_index of a cache the caller of decode() holds"""
    c = cache["cache_index"]
    for t in cache["k"] + cache["v"]:
        if c + 1 < t.shape[1]:
            poison_(t[:, c + 1:], how)
