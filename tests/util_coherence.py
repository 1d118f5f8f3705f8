"""Weight coherence: every copy derived from the fp32 master weights follows every way the weights can move.  Shared by
tests/test_coherence_gpu.py (the sweep {way the weights moved} x {derived copy} x {mode} on the device) and tests/test_coherence_cpu.py
(the comparison cores on numpy arrays with planted defects, and the completeness of the sweep).  A helper module, not a conftest.

The inventory (INVENTORY below: one row, one checker each).  engine.py, fp8_state.py, params.py, modeling_clip_vision_mbart.py and
generation_clip_vision_utils.py hold nothing else that caches a function of the weights across calls: `ParamStore._vcache` holds views
that alias the flat buffers, a decode plan holds search state and the addresses of the copies below, the cross-attention K/V of
`_decode_set_encoder` and `Fp8State.cache` / `saved` live for one call / one pass.

  lp        bf16 compute copy `ParamStore.lp`, the whole flat buffer (alignment padding and the embedding's pad rows included).
            Refreshed by `ParamStore.refresh_lp` (params setter, checkpoint restore) and by the `p_lp` output of every AdamW kernel.
            Check: bit for bit `util_gemm_ref.round_bf16(master)`; fp32 models: `lp is master`.
  shared_T  E^T, `Engine._bufs[("w.sharedT", d, Vpad, bf16)]`, the k-contiguous copy of the tied embedding (bf16, Vpad >= 16384).
            Refreshed by `Engine.refresh_shared_T` (aux stream + event, end of a train step) or on the spot by `Engine.shared_T`.
            Check: `util_rowop_ref.check_transposed` against `store.w("shared")` after `shared_T()` and a synchronise;
            `eng._ET_version == store.version`.
  ln_folds  `Engine._lnf[wname]` = (gamma o W, colsum, bias') of the decoder-step Linears behind a LayerNorm (bf16).  Refreshed by
            `Engine.ln_folded` (from `_decode_set_encoder`, once per generate call) when `ParamStore.version` moved.
            Check: bit for bit a fresh `ops.ln_fold_weight` into new buffers, and within `util_rowop_ref.fold_ref`'s bound; the tensors
            stay where they are (captured decoder steps hold their addresses).
  shortlist `Shortlist.E`, `.bias`: the gathered rows of the tied embedding / entries of final_logits_bias.  Refreshed by
            `Shortlist.refresh` (from `_shortlist_of`, once per generate call) when `ParamStore.version` moved.
            Check: bit for bit the gather, padding zero, `data_ptr` unchanged.
  fp8       `Fp8State.weights[n]` (q, qT, scale slot) of every fp8 Linear, `shared` and `ckvcat` included.  Refreshed by
            `Fp8State.refresh_weights` (aux stream, behind the optimizer) or `begin_pass`; readers go through `wait`.
            Check: `util_fp8_ref.quant_expect` + `check_quant` (bytes and both words of the scale slot) under the scale source that
            applies — current scaling, or a change not made by the optimizer: the current amax; delayed scaling behind an optimizer step:
            the amax of the weights before that step — and `qT` bit for bit `q.T`.  Read behind a pass (`eval_step`) and a synchronise.
  params    `model.params` (`_params_cache`).  Dropped by `invalidate_params_cache`, replaced by the params setter.
            Check: leaves equal `export_flat("master")`; a new object after any change.

The events (EVENTS below): the ways the weights move, one small driver each."""
from __future__ import annotations

import numpy as np

import util_fp8_ref as F8
import util_rowop_ref as RR
from util_gemm_ref import check, round_bf16

INVENTORY = ("lp", "shared_T", "ln_folds", "shortlist", "fp8", "params")

FP8_WIDTHS = dict(d_model=256, d_ffn=512, d_heads=4, v_hidden=256, v_ffn=512, v_heads=4)  # the fp8 head needs d % 128 == 0 beside 64-wide heads
WIDE_VOCAB = 16400  # Vpad = 16512 >= 16384: the bf16 head backward takes the NT launches and E^T exists (Engine._head_nt_kcap)

# mode -> storage dtype, overrides of util_small.SMALL, Trainer arguments, the inventory rows that exist in it
MODES = {
    "fp32": dict(dtype="float32", over={}, trainer={}, rows=("lp", "shortlist", "params")),
    "bf16": dict(dtype="bfloat16", over={}, trainer={}, rows=("lp", "ln_folds", "shortlist", "params")),
    "bf16wide": dict(dtype="bfloat16", over=dict(vocab_size=WIDE_VOCAB), trainer={}, rows=("lp", "shared_T", "ln_folds", "shortlist", "params")),
    "fp8delayed": dict(dtype="bfloat16", over=FP8_WIDTHS, trainer=dict(gemm_dtype="fp8", fp8_scaling="delayed"),
                       rows=("lp", "ln_folds", "shortlist", "fp8", "params")),
    "fp8current": dict(dtype="bfloat16", over=FP8_WIDTHS, trainer=dict(gemm_dtype="fp8", fp8_scaling="current"),
                       rows=("lp", "ln_folds", "shortlist", "fp8", "params")),
}
ALL, NO_FP8 = tuple(MODES), ("fp32", "bf16", "bf16wide")  # (Trainer refuses accumulation, clipping and groups beside fp8 GEMMs)
TWIN_MODES = ALL  # the black-box twin; fp8 trainers against a bf16 twin (their inference entry points run bf16)

GROUPS = [dict(match=r"vit.*|patch\.w", frozen=True), dict(match=r"dec\d+\..*", lr_scale=0.5)]

# event -> what it is, the modes it applies to, the Trainer arguments it needs, whether a checkpoint is saved ahead of the warm-up
EVENTS = {
    "E1_step": dict(what="train_step, overlapped per-bucket optimizer", modes=ALL, trainer={}),
    "E2_step_one_launch": dict(what="train_step, overlap_optimizer=False", modes=ALL, trainer=dict(overlap_optimizer=False)),
    "E3_accumulate": dict(what="accumulate_steps=2: nothing moves on the first micro-step", modes=NO_FP8, trainer=dict(accumulate_steps=2)),
    "E4_clip": dict(what="max_grad_norm=1.0", modes=NO_FP8, trainer=dict(max_grad_norm=1.0)),
    "E5_groups": dict(what="param_groups: frozen encoder and an lr_scale group", modes=NO_FP8, trainer=dict(param_groups=GROUPS)),
    "E6_setter": dict(what="model.params = another tree", modes=ALL, trainer={}),
    "E7_restore": dict(what="restore_checkpoint of a checkpoint saved two steps earlier", modes=ALL, trainer={}, checkpoint=True),
    "E8_raised": dict(what="a step that raised after some optimizer passes", modes=ALL, trainer={}),
    "E9_step_restore": dict(what="E1 then E7, no pass in between", modes=ALL, trainer={}, checkpoint=True),
    "E9_setter_step": dict(what="E6 then E1, no pass in between", modes=ALL, trainer={}),
}
MATRIX = [(m, e) for m in MODES for e, d in EVENTS.items() if m in d["modes"]]

GEN_BEAM = dict(max_length=6, num_beams=4)
GEN_GREEDY = dict(max_length=6, num_beams=1)
GEN_SAMPLE = dict(max_length=6, num_beams=1, do_sample=True, prng_key=7)
ALLOWED = np.array([2] + list(range(20, 60)), dtype=np.int32)  # EOS = forced EOS = 2 and 40 ordinary ids


# ================================================================================================ comparison cores (numpy only)
def bf16_bits(values) -> np.ndarray:
    """uint16 bits of values that are exact in bf16"""
    return (np.ascontiguousarray(values, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_values(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def _same_bits(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, f"{what}: {got.shape} {got.dtype} against {ref.shape} {ref.dtype}"
    bad = got != ref
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {i}: {got[i]!r} != {ref[i]!r}")


def core_lp(lp_bits, master):
    """lp (uint16 bits, the flat buffer) is round-to-nearest-even of master (float32, the flat buffer), bit for bit"""
    _same_bits(np.asarray(lp_bits, np.uint16), bf16_bits(round_bf16(np.asarray(master, np.float32))), "lp against round_bf16(master)")


def core_transposed(t_bits, src_bits):
    """t [d][Vpad] is the transpose of src [Vpad][d] (uint16 bits)"""
    rows = src_bits.shape[0]
    assert t_bits.shape == (src_bits.shape[1], rows), f"E^T: shape {t_bits.shape} for a source {src_bits.shape}"
    RR.check_transposed(t_bits, src_bits, rows, rows)


def core_fold(got, w, gamma, beta, bias, what, fresh=None):
    """got = (w_fold uint16 bits, colsum fp32, bias' fp32) of the bf16 weight w (values), LayerNorm gamma / beta and bias (fp32):
    w_fold is round(w * gamma) bit for bit, the two vectors lie within fold_ref's bounds; fresh: the same three from a fold made now,
    equal bit for bit"""
    wf, cs, bf = got
    if fresh is not None:
        _same_bits(wf, fresh[0], f"{what}: w_fold against a fresh fold")
        _same_bits(np.asarray(cs, np.float32).view(np.uint32), np.asarray(fresh[1], np.float32).view(np.uint32), f"{what}: colsum against a fresh fold")
        _same_bits(np.asarray(bf, np.float32).view(np.uint32), np.asarray(fresh[2], np.float32).view(np.uint32), f"{what}: bias' against a fresh fold")
    r_wf, r_cs, e_cs, r_bf, e_bf = RR.fold_ref(w, gamma, beta, bias, "bf16")
    _same_bits(np.asarray(wf, np.uint16), bf16_bits(r_wf), f"{what}: w_fold against round(w * gamma)")
    check(cs, r_cs, e_cs, f"{what}: colsum", log=False)
    check(bf, r_bf, e_bf, f"{what}: bias'", log=False)


def core_gather(E_bits, bias_bits, shared_bits, flb_bits, ids, what="shortlist"):
    """E [Ns_pad][d] = shared[ids], bias [Ns_pad] = flb[ids] (integer bits), padding zero"""
    n = len(ids)
    _same_bits(E_bits[:n], shared_bits[ids], f"{what}: gathered rows")
    _same_bits(bias_bits[:n], flb_bits[ids], f"{what}: gathered bias")
    assert not E_bits[n:].any() and not bias_bits[n:].any(), f"{what}: padding rows / entries are not zero"


def core_fp8(got, src, amax_old, what):
    """got = dict(q uint8 [N][K], qT uint8 [K][N], state fp32 [2]) of the bf16 weight src [N][K] (values) under the scale source
    amax_old (None: the weight's own amax)"""
    N, K = np.shape(src)
    exp = F8.quant_expect(src, N, K, N, "e4m3", amax_old)
    F8.check_quant(exp, got, what, "e4m3")
    _same_bits(np.asarray(got["qT"], np.uint8), np.ascontiguousarray(np.asarray(got["q"], np.uint8).T), f"{what}: qT against q.T")


def core_params(leaves, export, what="model.params"):
    """the flat leaves of model.params equal those exported from the master buffer now"""
    assert set(leaves) == set(export), f"{what}: leaf names differ"
    for k in export:
        a, b = np.asarray(leaves[k]), np.asarray(export[k])
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: leaf {k} is not what the master buffer holds"


# ================================================================================================ device side: read the copies
def _bits(t):
    """integer bits of a device tensor as numpy"""
    import torch

    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.float32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    if t.element_size() == 1:
        return t.view(torch.uint8).cpu().numpy()
    raise TypeError(t.dtype)


def _sync():
    import torch

    torch.cuda.synchronize()


def fold_names(store):
    """(Linear, LayerNorm) pairs whose folds a decoder step reads (`_decode_set_encoder`)"""
    out = []
    for l in range(store.L):
        p = f"dec{l}."
        for wn, ln in ((p + "qkv", p + "ln_sa"), (p + "cq", p + "ln_ca"), (p + "fc1", p + "ln_ff")):
            if l > 0 or not wn.endswith("qkv"):
                out.append((wn, ln))
    return out


def _et_key(model):
    import torch

    st = model.store
    return ("w.sharedT", st.d, st.Vpad, torch.bfloat16)


def check_lp(ctx, info):
    st = ctx.model.store
    _sync()
    if ctx.dtype_name == "float32":
        assert st.lp is st.master, "fp32 model: lp is not the master buffer"
        return
    assert st.lp is not st.master and st.lp.numel() == st.master.numel()
    core_lp(_bits(st.lp), st.master.cpu().numpy())


def check_shared_T(ctx, info):
    eng, st = ctx.model.engine, ctx.model.store
    ET = eng._bufs.get(_et_key(ctx.model))
    assert ET is not None, "E^T was never built: the head backward did not take the NT launches"
    got = eng.shared_T()
    _sync()
    assert got is ET and ET.data_ptr() == ctx.ptrs["shared_T"], "E^T moved"
    core_transposed(_bits(got[: st.d]), _bits(st.w("shared")))
    assert eng._ET_version == st.version, f"E^T belongs to version {eng._ET_version}, the weights are at {st.version}"


def _fold_arrays(triple):
    return _bits(triple[0]), triple[1].cpu().numpy(), triple[2].cpu().numpy()


def check_ln_folds(ctx, info):
    import torch

    from mic_amd import ops

    eng, P = ctx.model.engine, ctx.model.store
    for wn, ln in fold_names(P):
        assert wn in eng._lnf, f"the fold of {wn} was never built"
        hit = eng.ln_folded(wn, ln)  # the lazy refresh a generate call runs
        assert hit is eng._lnf[wn] and tuple(t.data_ptr() for t in hit) == ctx.ptrs["ln_folds"][wn], f"the fold of {wn} moved"
        w = P.w(wn + ".w")
        fresh = (torch.empty_like(w), torch.empty(w.shape[0], dtype=torch.float32, device=w.device),
                 torch.empty(w.shape[0], dtype=torch.float32, device=w.device))
        ops.ln_fold_weight(w, P.f32(ln + ".g"), P.f32(ln + ".b"), P.f32(wn + ".b"), *fresh)
        _sync()
        core_fold(_fold_arrays(hit), w.float().cpu().numpy(), P.f32(ln + ".g").cpu().numpy(), P.f32(ln + ".b").cpu().numpy(),
                  P.f32(wn + ".b").cpu().numpy(), f"ln fold {wn}", fresh=_fold_arrays(fresh))


def check_shortlist(ctx, info):
    P = ctx.model.store
    sls = list(ctx.model._shortlists.values())
    assert sls, "no shortlist was built"
    for sl in sls:
        sl.refresh()  # the lazy refresh a generate call runs (`_shortlist_of`)
        _sync()
        assert (sl.E.data_ptr(), sl.bias.data_ptr()) == ctx.ptrs["shortlist"][sl.key], "the shortlist's tensors moved"
        core_gather(_bits(sl.E), _bits(sl.bias), _bits(P.w("shared")), _bits(P.f32("flb")), sl.ids)


def fp8_region(store, name):
    """(flat offset, N, K) of the matrix behind the fp8 weight entry `name`"""
    if name == "ckvcat":
        return store.segs["dec0.ckv.w"].offset, store.L * 2 * store.d, store.d
    s = store.segs["shared" if name == "shared" else name + ".w"]
    return s.offset, s.shape[0], s.shape[1]


def check_fp8(ctx, info):
    """behind a pass and a synchronise: the pass's first fp8 GEMMs went through `Fp8State.wait()`"""
    eng, st = ctx.model.engine, ctx.model.store
    f8 = eng.f8
    ctx.tr.eval_step(ctx.bt)
    _sync()
    assert not f8.stale
    delayed_history = f8.delayed and info.get("by_optimizer") and info.get("pre_lp") is not None
    assert {"shared", "ckvcat"} <= set(f8.weights), sorted(f8.weights)
    for n, w8 in f8.weights.items():
        src = f8.src(n)
        off, N, K = fp8_region(st, n)
        assert tuple(src.shape) == (N, K) and src.data_ptr() == st.lp[off:].data_ptr()
        amax_old = None
        if delayed_history:  # the amax the previous quantiser pass recorded: that of the weights before the optimizer step
            amax_old = float(info["pre_lp"][off: off + N * K].float().abs().max().item())
        core_fp8(dict(q=_bits(w8.q), qT=_bits(w8.qT), state=w8.state.cpu().numpy()), src.float().cpu().numpy(), amax_old, f"fp8 copy of {n}")


def check_params(ctx, info):
    from mic_amd.params import flatten_tree

    _sync()
    tree = ctx.model.params
    assert tree is not ctx.params_before, "model.params is the object it was before the weights changed"
    core_params(flatten_tree(tree), ctx.model.store.export_flat("master"))


CHECKERS = dict(lp=check_lp, shared_T=check_shared_T, ln_folds=check_ln_folds, shortlist=check_shortlist, fp8=check_fp8, params=check_params)
assert tuple(CHECKERS) == INVENTORY


def run_checkers(ctx, info, rows=None, changed=True):
    """every checker of the inventory that applies to the mode; all failures are reported together.  changed=False: the weights have
    not moved (`params` may then be the object it was)."""
    errs = []
    for row in (rows or MODES[ctx.mode]["rows"]):
        if row == "params" and not changed:
            continue
        try:
            CHECKERS[row](ctx, info)
        except AssertionError as e:
            errs.append(f"[{ctx.mode} / {ctx.event} / {row}] {e}")
    assert not errs, "stale or wrong derived copies:\n" + "\n".join(errs)


# ================================================================================================ set-up
class Ctx:
    pass


def lr_fn():
    from mic_amd import create_learning_rate_fn

    return create_learning_rate_fn(64, 2, 4, 2, 2e-3)


def _batch_dict(rc):
    from util_small import batch

    px, labels, mask, dec_in = batch(rc, 3, 12, seed=9)
    return dict(pixel_values=px.numpy(), input_ids=labels.numpy(), attention_mask=mask.numpy(), decoder_input_ids=dec_in.numpy())


def record_ptrs(ctx):
    eng = ctx.model.engine
    ET = eng._bufs.get(_et_key(ctx.model))
    ctx.ptrs = dict(shared_T=None if ET is None else ET.data_ptr(),
                    ln_folds={wn: tuple(t.data_ptr() for t in trip) for wn, trip in eng._lnf.items()},
                    shortlist={sl.key: (sl.E.data_ptr(), sl.bias.data_ptr()) for sl in getattr(ctx.model, "_shortlists", {}).values()})


def prepare(mode, event, dev, tmp_path):
    """a model of `mode` under the Trainer `event` needs, warm: 2 train steps, a beam search called twice (the second call captures the
    plan's steps) and a shortlist beam search called twice — every derived copy of the mode exists and captured graphs point into them.
    MIC_DECODE_GRAPHS=1 is the caller's to set."""
    import torch

    from mic_amd import Trainer
    from util_small import make_pair

    md, ev = MODES[mode], EVENTS[event]
    assert mode in ev["modes"]
    ctx = Ctx()
    ctx.mode, ctx.event, ctx.dev, ctx.tmp, ctx.dtype_name = mode, event, dev, tmp_path, md["dtype"]
    ctx.dtype = getattr(torch, md["dtype"])
    ctx.rc, _, ctx.model = make_pair(ctx.dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0, **md["over"])
    ctx.tr = Trainer(ctx.model, lr_fn(), bucket_mb=0.25, **md["trainer"], **ev["trainer"])
    assert len(ctx.tr.buckets) > 2
    ctx.bt = _batch_dict(ctx.rc)
    ctx.px = ctx.bt["pixel_values"]
    ctx.calls_per_step = ev["trainer"].get("accumulate_steps", 1)
    ctx.ckpt = None
    if ev.get("checkpoint"):
        opt_step(ctx)
        ctx.ckpt, ctx.ckpt_step = ctx.tr.save_checkpoint(str(tmp_path), with_opt=True), ctx.tr.step
    eng = ctx.model.engine
    for i in range(2):
        opt_step(ctx)
        if i == 0 and "shared_T" in md["rows"]:
            assert eng._bufs.get(_et_key(ctx.model)) is not None, "the reduced wide-vocabulary model does not take the NT head backward"
    if "shared_T" not in md["rows"]:
        assert eng._bufs.get(_et_key(ctx.model)) is None
    for kw in (GEN_BEAM, dict(GEN_BEAM, allowed_token_ids=ALLOWED)):
        for _ in range(2):
            ctx.model.generate(ctx.px, **kw)
    ctx.plans = {k: (p, p.calls) for k, p in ctx.model._decode_plans.items()}
    assert len(ctx.plans) == 2 and all(len(p.graphs) > 0 and not p.streams for p, _ in ctx.plans.values()), "single-chain plans with captured steps"
    if "ln_folds" in md["rows"]:
        assert set(eng._lnf) == {wn for wn, _ in fold_names(ctx.model.store)}
    else:
        assert not eng._lnf
    assert (eng.f8 is not None) == ("fp8" in md["rows"])
    ctx.params_before = ctx.model.params  # (fills the cache)
    record_ptrs(ctx)
    _sync()
    return ctx


def opt_step(ctx):
    """train_step calls up to and including the next optimizer step"""
    for _ in range(ctx.calls_per_step):
        out = ctx.tr.train_step(ctx.bt)
    return out


def _master_bits(ctx):
    import torch

    _sync()
    return ctx.model.store.master.view(torch.int32).clone()


def _moved(ctx, before, what):
    import torch

    assert not torch.equal(_master_bits(ctx), before), f"{what}: the master weights did not move"


# ================================================================================================ events
def ev_step(ctx):
    """E1 / E2 / E4: one optimizer step of the Trainer as constructed"""
    before, pre_lp = _master_bits(ctx), ctx.model.store.lp.clone()
    v0 = ctx.model.store.version
    opt_step(ctx)
    _moved(ctx, before, "train_step")
    assert ctx.model.store.version > v0
    return dict(by_optimizer=True, pre_lp=pre_lp)


def snapshot_derived(ctx):
    """bits of every derived buffer that exists + the version each copy says it belongs to"""
    import torch

    eng, st = ctx.model.engine, ctx.model.store
    iv = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
    snap = {"lp": st.lp.view(iv[st.lp.dtype]).clone()}
    ET = eng._bufs.get(_et_key(ctx.model))
    if ET is not None:
        snap["shared_T"] = ET.view(torch.int16).clone()
    for wn, trip in eng._lnf.items():
        for i, t in enumerate(trip):
            snap[f"fold.{wn}.{i}"] = t.view(iv[t.dtype]).clone()
    for sl in getattr(ctx.model, "_shortlists", {}).values():
        snap[f"sl.{sl.key}.E"], snap[f"sl.{sl.key}.bias"] = sl.E.view(iv[sl.E.dtype]).clone(), sl.bias.view(torch.int32).clone()
    marks = (st.version, eng._ET_version, eng._lnf_version, tuple(sl.version for sl in getattr(ctx.model, "_shortlists", {}).values()))
    return snap, marks


def ev_accumulate(ctx):
    """E3: the first micro-step moves nothing — version, every checker, every derived buffer as it was; the second is the step"""
    import torch

    assert ctx.tr.accumulate_steps == 2 and ctx.tr._micro == 0
    run_checkers(ctx, {}, changed=False)  # (brings the lazily refreshed copies up to date with the warm-up's last step)
    before = _master_bits(ctx)
    snap, marks = snapshot_derived(ctx)
    params = ctx.model.params
    ctx.tr.train_step(ctx.bt)
    assert ctx.tr._micro == 1
    assert torch.equal(_master_bits(ctx), before), "the first micro-step of an accumulation moved the master weights"
    run_checkers(ctx, {}, changed=False)
    snap2, marks2 = snapshot_derived(ctx)
    assert marks2 == marks, f"the first micro-step of an accumulation moved a version: {marks} -> {marks2}"
    assert set(snap2) == set(snap)
    for k in snap:
        assert torch.equal(snap[k], snap2[k]), f"the first micro-step of an accumulation rewrote {k}"
    assert ctx.model.params is params
    pre_lp = ctx.model.store.lp.clone()
    ctx.tr.train_step(ctx.bt)
    assert ctx.tr._micro == 0
    _moved(ctx, before, "the second micro-step")
    return dict(by_optimizer=True, pre_lp=pre_lp)


def ev_groups(ctx):
    """E5: frozen segments keep their master and lp bits, every other weight matrix moved"""
    import re

    import torch

    from mic_amd.train import ENCODER

    st = ctx.model.store
    iv = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
    before, lp0 = _master_bits(ctx), st.lp.view(iv[st.lp.dtype]).clone()
    pre_lp = st.lp.clone()
    opt_step(ctx)
    after, lp1 = _master_bits(ctx), st.lp.view(iv[st.lp.dtype])
    frozen = 0
    for name, s in st.segs.items():
        a, b = s.offset, s.offset + s.numel
        if re.fullmatch(ENCODER, name):
            frozen += 1
            assert torch.equal(after[a:b], before[a:b]) and torch.equal(lp1[a:b], lp0[a:b]), f"frozen segment {name} changed"
        elif name.endswith(".w") or name == "shared":
            assert not torch.equal(after[a:b], before[a:b]), f"segment {name} is not frozen and did not move"
    assert frozen > 10
    return dict(by_optimizer=True, pre_lp=pre_lp)


def other_tree(model):
    """a parameter tree different from the model's in every leaf"""
    from mic_amd.params import flatten_tree, unflatten_tree

    return unflatten_tree({k: (np.asarray(v, np.float32) * np.float32(1.03125) + np.float32(2.0 ** -7)) for k, v in flatten_tree(model.params).items()})


def ev_setter(ctx):
    """E6"""
    before = _master_bits(ctx)
    ctx.model.params = other_tree(ctx.model)
    _moved(ctx, before, "the params setter")
    return dict(by_optimizer=False, pre_lp=None)


def ev_restore(ctx, steps_first=2):
    """E7: into the same trainer, the checkpoint `prepare` saved ahead of the warm-up's two steps"""
    assert ctx.ckpt is not None and ctx.tr.step == ctx.ckpt_step + steps_first
    before = _master_bits(ctx)
    assert ctx.tr.restore_checkpoint(ctx.ckpt) == ctx.ckpt_step
    _moved(ctx, before, "restore_checkpoint")
    return dict(by_optimizer=False, pre_lp=None)


def ev_raised(ctx):
    """E8: `reducer.finish` raises a Python exception — backward has run and the per-bucket optimizer passes it released have been
    issued; never a device fault"""
    tr = ctx.tr
    before = _master_bits(ctx)

    def failing(*a, **kw):
        raise RuntimeError("finish failed")
    tr.reducer.finish = failing
    try:
        tr.train_step(ctx.bt)
    except RuntimeError as e:
        assert "finish failed" in str(e)
    else:
        raise AssertionError("the step did not raise")
    finally:
        del tr.reducer.finish
    eng = ctx.model.engine
    assert eng.on_embed_rows is None and eng.grad_progress is None
    _moved(ctx, before, "the optimizer passes issued before the step raised")
    return dict(by_optimizer=False, pre_lp=None)


def ev_step_restore(ctx):
    """E9: E1 then E7 — the side-stream refreshes of the step's version may still be in flight"""
    ev_step(ctx)
    return ev_restore(ctx, steps_first=3)


def ev_setter_step(ctx):
    """E9: E6 then E1"""
    ev_setter(ctx)
    return ev_step(ctx)


DRIVERS = {"E1_step": ev_step, "E2_step_one_launch": ev_step, "E3_accumulate": ev_accumulate, "E4_clip": ev_step, "E5_groups": ev_groups,
           "E6_setter": ev_setter, "E7_restore": ev_restore, "E8_raised": ev_raised, "E9_step_restore": ev_step_restore,
           "E9_setter_step": ev_setter_step}


# ================================================================================================ black-box twin
def twin_of(ctx):
    """a fresh model of the same storage dtype holding A's weights, and a maker of a default Trainer on it"""
    from mic_amd import FlaxCLIPVisionMBartForConditionalGeneration, Trainer
    from util_small import product_config

    B = FlaxCLIPVisionMBartForConditionalGeneration(product_config(ctx.rc), seed=0, dtype=ctx.dtype, device=ctx.dev)
    B.params = ctx.model.params
    return B, (lambda: Trainer(B, lr_fn()))


def check_twin(ctx):
    """A (warm plans, captured steps, whatever its copies hold) against the twin, bit for bit"""
    import torch

    A = ctx.model
    B, trainer_B = twin_of(ctx)
    bt = ctx.bt
    ea, eb = A.encode(ctx.px), B.encode(ctx.px)
    assert torch.equal(ea.last_hidden_state, eb.last_hidden_state), "encode"
    la = A.decode(bt["decoder_input_ids"], ea, decoder_attention_mask=bt["attention_mask"]).logits
    lb = B.decode(bt["decoder_input_ids"], eb, decoder_attention_mask=bt["attention_mask"]).logits
    assert torch.isfinite(la.float()).all() and torch.equal(la, lb), "teacher-forced decode"
    if ctx.model.engine.f8 is None:  # (an fp8 trainer's eval_step runs fp8 GEMMs: no bf16 twin computes its loss)
        assert torch.equal(ctx.tr.eval_step(bt)["loss"], trainer_B().eval_step(bt)["loss"]), "eval_step loss"
    # the two warm plans first: they are replayed, not rebuilt
    for kw in (GEN_BEAM, dict(GEN_BEAM, allowed_token_ids=ALLOWED)):
        oa, ob = A.generate(ctx.px, **kw), B.generate(ctx.px, **kw)
        assert torch.equal(oa.sequences, ob.sequences) and torch.equal(oa.scores, ob.scores), ("beam search", sorted(kw), oa.sequences, ob.sequences)
    for key, (plan, calls) in ctx.plans.items():
        assert A._decode_plans.get(key) is plan and plan.calls == calls + 1 and len(plan.graphs) > 0, "A did not replay its decode plan"
    assert all(p is not q for p in B._decode_plans.values() for q, _ in ctx.plans.values())
    oa, ob = A.generate(ctx.px, **GEN_GREEDY), B.generate(ctx.px, **GEN_GREEDY)
    assert torch.equal(oa.sequences, ob.sequences), "greedy search"
    oa, ob = A.generate(ctx.px, **GEN_SAMPLE), B.generate(ctx.px, **GEN_SAMPLE)
    assert torch.equal(oa.sequences, ob.sequences), "sampling"
    if oa.get("scores") is not None:
        assert torch.equal(oa.scores, ob.scores), "sampling scores"
