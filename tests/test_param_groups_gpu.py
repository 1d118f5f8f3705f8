"""Trainer(param_groups=...) on the MI355X: the grouped AdamW kernel (csrc/optimizer_groups.hip) against per-run launches of its
sibling mic_adamw and against the fp64 reference of tests/util_rowop_ref.py, then the Trainer — a catch-all group against the plain
Trainer, grouped steps against the oracle stepped per leaf, and a frozen image tower with and without its backward.

Every figure an assertion bounds is printed first ("[groups] ...")."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import util_rowop_cases as RC  # noqa: E402
import util_rowop_ref as RR  # noqa: E402
from test_rowop_conformance_gpu import F32, _adamw_bufs, twice  # noqa: E402
from util_gemm_ref import check  # noqa: E402
from util_small import batch, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------- kernel
N = 4096
R0, R1 = 64, 64 + 1024            # runs of 64 / 1 024 / the rest
SA, SB, SC = (1.0, 0.01), (0.5, 0.0), (2.0, 0.05)   # (lr_scale, wd) of three live groups
FZ = (0.0, 0.0, True)
BIG = 8192 * 1024 + 256           # a run longer than one trip of the 8192 x 256 x 4 grid: the grid-stride loop wraps


def _table(kind, n=N):
    live = lambda s: (s[0], s[1], False)  # noqa: E731
    if kind == "catch_all":
        return [(0, n) + live(SA)]
    if kind == "big":  # 64 frozen elements, then one run of n - 64 > 8192 * 1024
        return [(0, R0) + FZ, (R0, n) + live(SC)]
    three = {"live": (live(SA), live(SB), live(SC)), "frozen_first": (FZ, live(SB), live(SC)), "frozen_middle": (live(SA), FZ, live(SC)),
             "frozen_last": (live(SA), live(SB), FZ), "lr0_middle": (live(SA), (0.0, 0.01, False), live(SC))}[kind]
    return [(0, R0) + three[0], (R0, R1) + three[1], (R1, n) + three[2]]


# (table, slice [begin, end) of the buffer, what it is there for)
CASES = {
    "live": ("live", 0, N),
    "frozen_first": ("frozen_first", 0, N),
    "frozen_middle": ("frozen_middle", 0, N),
    "frozen_last": ("frozen_last", 0, N),
    "inside_runs": ("live", 20, N - 36),                 # begins inside the first run, ends inside the last
    "inside_runs_frozen_middle": ("frozen_middle", 20, N - 36),
    "within_one_run": ("live", 128, 1000),               # never crosses a boundary
    "wholly_frozen": ("frozen_middle", 128, 1000),       # no launch at all
    "catch_all": ("catch_all", 0, N),
    "lr_scale_0_is_not_frozen": ("lr0_middle", 0, N),
    "grid_stride": ("big", 0, BIG),
}


def _pieces(runs, b, e):
    """the runs clipped to [b, e): (lo, hi, lr_scale, wd, frozen), offsets relative to the buffer"""
    return [(max(rb, b), min(re_, e), s, w, f) for (rb, re_, s, w, f) in runs if rb < e and re_ > b]


@pytest.mark.parametrize("lp", [True, False], ids=["bf16_copy", "no_copy"])
@pytest.mark.parametrize("name", list(CASES))
def test_adamw_groups_is_bitwise_adamw_per_run(dev, name, lp):
    """one mic_adamw_groups launch over the slice = one mic_adamw launch per live run (hyper[0] pre-multiplied in fp32, the run's wd),
    bit for bit in p, m, v and p_lp; frozen runs and everything outside the windows keep their bytes; two launches over the same
    bytes give the same bits; and the result lies within the fp64 reference's own bounds"""
    from mic_amd import ops

    kind, b, e = CASES[name]
    n_buf = BIG if kind == "big" else N
    runs, n = _table(kind, n_buf), e - b
    c = RC.ADAMW_BY["adamw_4100_gs"]  # t = 7, lr = 1e-3, grad_scale = 0.5
    h = RC.adamw_hyper(c)
    p, m, v, g = RC.adamw_inputs(c, n)
    table = ops.AdamwRuns(runs, dev)
    hy = torch.tensor([h["lr"], h["t"]], dtype=F32, device=dev)
    pieces = _pieces(runs, b, e)
    live = np.zeros(n, bool)
    for (lo, hi, _, _, f) in pieces:
        live[lo - b:hi - b] = not f

    pb, mb, vb, gb, lpb, prep = _adamw_bufs(n, dev, p, m, v, g, lp=lp)
    outs = [o for o in (pb, mb, vb, lpb) if o is not None]
    launched = []
    twice(lambda: launched.append(ops.adamw_groups(table, b, pb.t[0], mb.t[0], vb.t[0], gb.t[0], lpb.t[0] if lpb else None, hy, h["b1"], h["b2"],
                                                   h["eps"], grad_scale=h["gscale"], n=n)), outs, name, prep=prep)
    assert launched == [bool(live.any())] * 2, "a wholly frozen slice launches nothing, every other slice launches once"
    for o in (pb, mb, vb):
        o.check_canary(name)
    if lpb:
        lpb.check_canary(name + " p_lp: frozen elements", torch.from_numpy(live.reshape(1, -1)))

    # the sibling, one launch per live run, on buffers of the same layout
    pb2, mb2, vb2, gb2, lpb2, prep2 = _adamw_bufs(n, dev, p, m, v, g, lp=lp)
    prep2()
    for (lo, hi, s, w, f) in pieces:
        if f:
            continue
        hy_r = torch.tensor([np.float32(h["lr"]) * np.float32(s), h["t"]], dtype=F32, device=dev)  # ONE fp32 multiply
        sl = slice(lo - b, hi - b)
        ops.adamw(pb2.t[0][sl], mb2.t[0][sl], vb2.t[0][sl], gb2.t[0][sl], lpb2.t[0][sl] if lpb2 else None, hy_r, h["b1"], h["b2"], h["eps"], w,
                  grad_scale=h["gscale"], n=hi - lo)
    torch.cuda.synchronize()
    for a, a2, k in ((pb, pb2, "p"), (mb, mb2, "m"), (vb, vb2, "v"), (lpb, lpb2, "p_lp")):
        if a is not None:
            assert torch.equal(a.bits(), a2.bits()), f"{name}: {k} differs from the per-run mic_adamw launches"

    # frozen bytes, and what moved
    idx = np.arange(n) if n <= 10000 else np.unique(np.concatenate([np.arange(4100), np.arange(n - 4100, n),
                                                                    np.random.default_rng(1).integers(n, size=100000)]))
    got = {k: bf.t[0].double().cpu().numpy() for k, bf in (("p", pb), ("m", mb), ("v", vb))}
    for k, a in (("p", p), ("m", m), ("v", v)):
        assert np.array_equal(got[k][~live], a[~live]), f"{name}: {k} of a frozen run moved"
        if live.any():
            assert not np.array_equal(got[k][live], a[live]) or (k == "p" and kind == "lr0_middle")
    if kind == "lr0_middle":  # lr_scale = 0: p keeps its bits, the moments move
        mid = slice(R0, R1)
        assert np.array_equal(got["p"][mid], p[mid]) and not np.array_equal(got["m"][mid], m[mid]) and not np.array_equal(got["v"][mid], v[mid])
    # against the fp64 reference at its own bounds, run by run
    for (lo, hi, s, w, f) in pieces:
        if f:
            continue
        ix = idx[(idx >= lo - b) & (idx < hi - b)]
        hr = dict(h, lr=float(np.float32(h["lr"]) * np.float32(s)), wd=w)
        r = RR.adamw_ref(p[ix], m[ix], v[ix], g[ix], **hr)
        for k in ("p", "m", "v"):
            assert np.isfinite(got[k][ix]).all()
            check(got[k][ix], r[k], r["bound_" + k], f"adamw_groups {k}: {name} run [{lo}, {hi})")
    if lpb:
        lv = torch.from_numpy(live).to(dev)
        assert torch.equal(lpb.t[0][lv], pb.t[0].to(torch.bfloat16)[lv]), f"{name}: p_lp is not the bf16 rounding of the stored p"


def test_adamw_groups_refusals_write_nothing(dev):
    from mic_amd import _lib, ops

    n = 256
    table = ops.AdamwRuns(_table("live"), dev)
    hy = torch.tensor([1e-3, 1.0], dtype=F32, device=dev)
    p, m, v, g = (torch.zeros(n + 8, device=dev) for _ in range(4))
    for bad in (lambda: ops.adamw_groups(table, 0, p[:n], m[:n], v[:n], g[:n], None, hy, 0.9, 0.999, 1e-8, n=n + 4),        # tensors too short
                lambda: ops.adamw_groups(table, N - 128, p[:n], m[:n], v[:n], g[:n], None, hy, 0.9, 0.999, 1e-8, n=n),     # past the table
                lambda: ops.adamw_groups(table, 0, p[:n], m[:n], v[:n], g[:n], None, hy, 0.9, 0.999, 1e-8, n=n - 2),        # n % 4
                lambda: ops.adamw_groups(table, 2, p[:n], m[:n], v[:n], g[:n], None, hy, 0.9, 0.999, 1e-8, n=n - 4),        # offset % 4
                lambda: ops.adamw_groups(table, 0, p[1:n + 1], m[:n], v[:n], g[:n], None, hy, 0.9, 0.999, 1e-8, n=n)):      # 4 bytes off a 16-byte boundary
        with pytest.raises(_lib.MicError):
            bad()
    for runs in ([], [(0, 64, 1.0, 0.0, False), (128, 256, 1.0, 0.0, False)], [(0, 62, 1.0, 0.0, False)]):  # empty, a gap, a ragged boundary
        with pytest.raises(_lib.MicError):
            ops.AdamwRuns(runs, dev)
    torch.cuda.synchronize()
    assert not p.any() and not m.any() and not v.any()


# ---------------------------------------------------------------------------------------------------------------- Trainer
B, T, STEPS, LR, WD = 4, 12, 3, 1e-3, 0.01


def _groups():
    from mic_amd.train import ENCODER, NO_DECAY

    return [dict(match=ENCODER, frozen=True), dict(match=NO_DECAY, weight_decay=0.0), dict(match=r"dec\d+\..*\.w", lr_scale=0.5)]


def _lr_fn():
    from mic_amd import create_learning_rate_fn

    return create_learning_rate_fn(train_ds_size=40, train_batch_size=4, num_train_epochs=1, num_warmup_steps=2, learning_rate=LR)


def _as_batch(b):
    px, labels, mask, dec_in = b
    return {"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}


def _make(dev, dtype, env=None, **kw):
    """a fresh reduced model and its Trainer (environment switches in `env` in force while it is built), clones of the initial state"""
    from mic_amd import Trainer

    keep = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
        st = model.store
        tr = Trainer(model, _lr_fn(), weight_decay=WD, label_smoothing_factor=0.0, seed=42, bucket_mb=0.25, **kw)
    finally:
        for k, val in keep.items():
            os.environ.pop(k, None) if val is None else os.environ.__setitem__(k, val)
    first = dict(master=st.master.clone(), lp=st.lp.clone(), m=st.m.clone(), v=st.v.clone())
    return dict(tr=tr, rc=rc, p=p, model=model, first=first, outs=[], losses=[], lines=[], grads=[])


def _step(run, s, trace=False, keep_grad=False):
    """train step s (the batch of seed 100 + s); trace: its launch sequence joins run["lines"]; keep_grad: a clone of the gradient
    buffer the optimizer consumed joins run["grads"]"""
    from util_step_trace import Recorder

    b = _as_batch(batch(run["rc"], B, T, seed=100 + s))
    if trace:
        with Recorder() as rec:
            out = run["tr"].train_step(b)
        run["lines"] += rec.events
    else:
        out = run["tr"].train_step(b)
    if keep_grad:
        run["grads"].append(run["model"].store.grad.clone())
    run["outs"].append(out)
    run["losses"].append(out["loss"].clone())
    return out


def _run(dev, dtype, trace=False, env=None, keep_grad=False, **kw):
    """STEPS train steps (seeds 100 ..) of a fresh reduced model"""
    run = _make(dev, dtype, env=env, **kw)
    for s in range(STEPS):
        _step(run, s, trace=trace, keep_grad=keep_grad)
    torch.cuda.synchronize()
    return run


def _copy_state(dst, src):
    """dst's weights, compute copy and moments := src's, bit for bit (what Trainer.restore_checkpoint does with a checkpoint's)"""
    a, b = src["model"].store, dst["model"].store
    for k in ("master", "m", "v"):
        getattr(b, k).copy_(getattr(a, k))
    if b.lp is not b.master:
        b.lp.copy_(a.lp)
    dst["model"].invalidate_params_cache()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _replay(run, grads, losses):
    """make run's engine hand its Trainer RECORDED gradients instead of computing them: the gradient buffer is filled on the step's
    stream, then every segment is reported final in flat order (what backward's `_done` calls do), so the reducer issues every
    bucket's optimizer pass, `finish()` the ones that wait for the end — all of the Trainer's own wiring, none of the backward's
    run-to-run noise"""
    eng, st = run["model"].engine, run["model"].store
    k = [0]

    def loss_and_grads(*a, **kw):
        st.grad.copy_(grads[k[0]])
        for seg in sorted(st.segs.values(), key=lambda x: x.offset):
            if eng.grad_progress is not None:
                eng.grad_progress(seg.offset + seg.numel)
        k[0] += 1
        return losses[k[0] - 1]

    eng.loss_and_grads = loss_and_grads


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_one_catch_all_group_is_the_plain_trainer(dev, dtype):
    """one catch-all group (1.0, wd): master, m, v (and the compute copy) bit for bit those of a plain Trainer whose tied embedding is
    not split by rows (MIC_OPT_SPLIT_SHARED=0), over 3 steps.

    Two independent runs of ANY Trainer — the plain one against itself included — do not agree bit for bit: the gradients accumulated
    with fp32 atomics (flb, the scattered rows of the tied embedding, the atomic region) depend on the order the adds land in, and from
    the second step on that noise is in every weight.  Measured on the MI355X over these 3 steps: two runs of the plain Trainer differ
    in 114 027 of 920 320 master elements in fp32 (max 4.2e-7) and in 8 in bf16 (max 3.7e-9); catch-all against plain, both computing
    their own gradients, in 106 569 (max 6.7e-7) and 17 (max 1.9e-9) — the same noise.  So the grouped Trainer is handed the
    very gradients the plain one consumed (`_replay`: its engine's loss_and_grads fills the buffer and reports every segment; buckets,
    streams, ordering rules, finish() and the kernels are the Trainer's own), and the comparison is bit for bit on every element.  The
    same grouped Trainer computing its own gradients is held to the run-to-run bounds of
    test_clip_gpu.py::test_infinite_max_norm_measures_and_is_the_default_trainer."""
    plain = _run(dev, dtype, env={"MIC_OPT_SPLIT_SHARED": "0"}, keep_grad=True)
    groups = [dict(match=".*", lr_scale=1.0, weight_decay=WD)]
    one = _make(dev, dtype, param_groups=groups)
    _replay(one, plain["grads"], plain["losses"])
    for s in range(STEPS):
        _step(one, s)
    torch.cuda.synchronize()
    assert not plain["tr"]._split_shared and plain["tr"]._groups is None and plain["tr"].reducer.on_ready is not None
    assert one["tr"]._groups is not None and one["tr"]._group_runs == [(0, one["model"].store.numel, 1.0, WD, False)]
    assert not one["tr"]._split_shared and one["tr"].reducer.on_ready is not None and len(one["tr"].buckets) > 3
    sa, sb = plain["model"].store, one["model"].store
    assert not torch.equal(sa.master, plain["first"]["master"]) and sa.m.any() and sa.v.any()
    for k in ("master", "m", "v", "lp"):
        a, b = getattr(sa, k), getattr(sb, k)
        nd = int((_bits(a) != _bits(b)).sum())
        print(f"[groups] catch-all (replayed gradients) vs plain {dtype} {k}: {nd} of {a.numel()} elements differ")
        assert nd == 0, k
    for o in one["outs"]:
        assert set(o) == {"loss", "learning_rate"}
    # the same Trainer on its own gradients: within the run-to-run noise of two default Trainers
    own = _run(dev, dtype, param_groups=groups)
    so = own["model"].store
    diff = (so.master - sa.master).abs()
    print(f"[groups] catch-all (own gradients) vs plain {dtype}: master {int((_bits(so.master) != _bits(sa.master)).sum())} of {diff.numel()} "
          f"elements differ, max {diff.max().item():.3e}, share > 1e-6 {(diff > 1e-6).float().mean().item():.2e}")
    assert np.allclose([x.item() for x in own["losses"]], [x.item() for x in plain["losses"]], rtol=1e-5)
    assert diff.max().item() <= 2.5 * LR * STEPS and (diff > 1e-6).float().mean().item() < 1e-3
    for k in ("m", "v"):
        d = (getattr(so, k) - getattr(sa, k)).abs().max().item()
        assert d <= 1e-3 * getattr(sa, k).abs().max().item(), (k, d)


def _leaf_groups(st, groups, wd):
    """{flax leaf: (lr_scale, wd, frozen)} — every leaf of a segment belongs to the segment's group"""
    from mic_amd.train import _segment_groups

    per = {name: (s, w, f) for (name, _, s, w, f) in _segment_groups(st, groups, wd)}
    return {leaf: per[seg] for seg, parts in st._mapping() for (leaf, _) in parts}


_ORACLE = {}


def _oracle_steps(rc, p, leaf_groups):
    """the oracle stepped per leaf: train_ref.adamw_update(lr_t * scale, wd_group), a frozen leaf left alone (optax.set_to_zero);
    computed once per grouping (the initial parameters are those of util_small.SEED in every test here)"""
    key = tuple(sorted(leaf_groups.items()))
    if key not in _ORACLE:
        _ORACLE[key] = _oracle_steps_once(rc, p, leaf_groups)
    return _ORACLE[key]


def _oracle_steps_once(rc, p, leaf_groups):
    from oracle import train_ref

    params = {k: x.clone() for k, x in p.items()}
    m = {k: torch.zeros_like(x) for k, x in p.items()}
    v = {k: torch.zeros_like(x) for k, x in p.items()}
    losses, lrs = [], []
    for step in range(STEPS):
        px, labels, mask, dec_in = batch(rc, B, T, seed=100 + step)
        loss, g = train_ref.loss_and_grads(rc, params, px, labels, mask, dec_in)
        lr = train_ref.linear_warmup_decay(step, LR, 2, 10)
        losses.append(loss.item())
        lrs.append(lr)
        for k in params:
            scale, wd, frozen = leaf_groups[k]
            if not frozen:
                params[k], m[k], v[k] = train_ref.adamw_update(params[k], g[k], m[k], v[k], step, lr * scale, wd=wd)
    return params, losses, lrs


def test_grouped_steps_match_the_oracle_stepped_per_leaf(dev):
    """{ENCODER frozen, NO_DECAY wd 0, decoder weights lr_scale 0.5}, 3 steps under warmup: every leaf within 2e-5 absolute (the bound
    of test_model_gpu.py::test_train_steps_match_oracle_adamw) of the oracle stepped per leaf; frozen leaves byte-identical to their
    initial master, compute copy, m, v; and the same run does NOT match the ungrouped oracle"""
    from mic_amd.params import flatten_tree

    run = _run(dev, torch.float32, param_groups=_groups())
    tr, st, rc, p = run["tr"], run["model"].store, run["rc"], run["p"]
    assert tr._encoder_frozen and tr.skip_frozen_backward
    lg = _leaf_groups(st, _groups(), WD)
    assert {x for x in lg.values()} == {(1.0, WD, False), (1.0, 0.0, False), (0.5, WD, False), (1.0, WD, True)}
    ref, ref_losses, lrs = _oracle_steps(rc, p, lg)
    for o, rl, lr in zip(run["outs"], ref_losses, lrs):
        assert abs(float(o["learning_rate"]) - lr) < 1e-9, "the returned learning rate stays the base rate"
        assert abs(float(o["loss"]) - rl) < 5e-5 * max(1.0, rl)
    got = flatten_tree(run["model"].params)
    dist = {k: (torch.from_numpy(got[k]) - rv).abs().max().item() for k, rv in ref.items()}
    worst = max(dist, key=dist.get)
    print(f"[groups] grouped oracle: worst leaf {worst} {dist[worst]:.3e} (bound 2e-5)")
    assert all(d < 2e-5 for d in dist.values()), sorted(dist.items(), key=lambda kv: -kv[1])[:5]
    # frozen runs: not a byte of master, compute copy, m, v has changed
    frozen = [(b, e) for (b, e, _, _, f) in tr._group_runs if f]
    assert len(frozen) == 3
    for (b, e) in frozen:
        for k, buf in (("master", st.master), ("lp", st.lp), ("m", st.m), ("v", st.v)):
            assert torch.equal(_bits(buf[b:e]), _bits(run["first"][k][b:e])), (k, b, e)
    live = [(b, e) for (b, e, _, _, f) in tr._group_runs if not f]
    assert all(not torch.equal(st.m[b:e], run["first"]["m"][b:e]) for (b, e) in live)
    # the control: against the ungrouped oracle (one AdamW over every leaf) the same weights must miss the bound
    plain, _, _ = _oracle_steps(rc, p, {k: (1.0, WD, False) for k in p})
    dist0 = {k: (torch.from_numpy(got[k]) - rv).abs().max().item() for k, rv in plain.items()}
    missed = {k: d for k, d in dist0.items() if not d < 2e-5}
    print(f"[groups] ungrouped oracle: {len(missed)} of {len(dist0)} leaves miss 2e-5, worst {max(dist0.values()):.3e}")
    assert missed, "an ignored param_groups argument would pass the grouped comparison"
    assert any(lg[k][2] for k in missed) and any(lg[k][0] == 0.5 for k in missed)


# what only the ViT's backward launches (the decoder has attention / LayerNorm backward of its own: those are counted)
VIT_ONLY = ("mic_vit_assemble_bwd",)
COUNTED = ("mic_attn_bwd", "mic_attn_bwd_packed", "mic_attn_bwd_packed_tiled", "mic_layernorm_bwd", "mic_layernorm_bwd_partials", "mic_gemm",
           "mic_gemm_grouped", "mic_vit_assemble_bwd")


def _name(line):
    m = re.match(r"(\w+)\(", line)
    return m.group(1) if m else ""


def _counts(lines):
    names = [_name(ln) for ln in lines]
    return {k: names.count(k) for k in COUNTED}


def _id_rows(run, s):
    """rows of the tied embedding that step s's decoder input ids scatter a gradient into (atomic adds)"""
    _, _, mask, dec_in = batch(run["rc"], B, T, seed=100 + s)
    return torch.unique(dec_in[mask.bool()] if run["tr"]._pack is not None else dec_in)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_skipping_the_frozen_towers_backward_changes_nothing_that_is_kept(dev, dtype):
    """skip_frozen_backward=True against False under the same groups, 3 steps: per-step loss bitwise equal; the GEMM-written
    non-encoder weights bit for bit; what is accumulated with fp32 atomics within 2e-5 of its scale (the bound of
    test_model_gpu.py::test_weight_gradient_stream_gives_the_same_gradients, both dtypes); the frozen segments untouched in both;
    and the launch sequence shows that no ViT backward kernel ran.

    The two Trainers run in lock-step: the full-backward one takes its 3 steps, and in front of every step the skipping one is given
    its state bit for bit (`_copy_state`).  Without that the comparison measures something else: the atomically accumulated gradients
    differ from run to run in their last bits, and from the second step on that noise is in every weight of BOTH runs (measured
    without the copy: after 3 steps 39 elements of flb differ in fp32, 15 of `shared` in bf16 — as between two runs of one Trainer).
    "GEMM-written": every .w segment of the dense region and the rows of `shared` this step's decoder ids do not touch; flb (a column
    sum) and the touched rows of `shared` (an atomic scatter) are held to the atomic region's bound."""
    from mic_amd.train import ENCODER

    full = _make(dev, dtype, param_groups=_groups(), skip_frozen_backward=False)
    skip = _make(dev, dtype, param_groups=_groups())
    sa, sb = full["model"].store, skip["model"].store
    assert skip["tr"]._encoder_frozen and skip["tr"].skip_frozen_backward and not full["tr"].skip_frozen_backward
    sh = sa.segs["shared"]
    worst = (0.0, None)
    for s in range(STEPS):
        _copy_state(skip, full)
        _step(full, s, trace=True)
        _step(skip, s, trace=True)
        torch.cuda.synchronize()
        assert not skip["model"].engine.skip_vit_backward, "the switch is set for the duration of a step only"
        la, lb = full["losses"][s], skip["losses"][s]
        print(f"[groups] skip vs full {dtype} step {s}: loss {la.item():.9g} {lb.item():.9g}")
        assert torch.equal(_bits(la), _bits(lb)), (s, la.item(), lb.item())
        touched = torch.zeros(sh.shape[0], dtype=torch.bool, device=dev)
        touched[_id_rows(full, s).to(dev)] = True
        for name, seg in sorted(sa.segs.items(), key=lambda kv: kv[1].offset):
            a, b = sa.f32(name), sb.f32(name)
            atomic = seg.offset >= sa.atomic_begin or name == "flb"
            if re.fullmatch(ENCODER, name):
                for st_, run in ((sa, full), (sb, skip)):
                    sl = slice(seg.offset, seg.offset + seg.numel)
                    assert all(torch.equal(_bits(getattr(st_, k)[sl]), _bits(run["first"][k][sl])) for k in ("master", "lp", "m", "v")), name
                continue
            if name == "shared":
                nd = int((_bits(a[~touched]) != _bits(b[~touched])).sum())
                assert nd == 0, (s, name, nd)
                a, b, atomic = a[touched], b[touched], True
            if not atomic:
                sl = slice(seg.offset, seg.offset + seg.numel)
                nd = [int((_bits(x[sl]) != _bits(y[sl])).sum()) for x, y in ((sa.master, sb.master), (sa.m, sb.m), (sa.v, sb.v), (sa.lp, sb.lp))]
                assert nd == [0, 0, 0, 0], (s, name, nd)
            else:
                scale = a.abs().max().item()
                d = (a - b).abs().max().item()
                if scale > 0 and d / scale > worst[0]:
                    worst = (d / scale, f"step {s} {name}")
                assert d <= 2e-5 * scale, (s, name, d, scale)
    vp = slice(sa.segs["vp.w"].offset, sa.segs["vp.w"].offset + sa.segs["vp.w"].numel)
    assert not torch.equal(sb.master[vp], skip["first"]["master"][vp]), "the bridge still trains"
    print(f"[groups] skip vs full {dtype} atomically accumulated segments: worst |d| / scale {worst[0]:.3e} ({worst[1]}; bound 2e-5)")
    # the launch sequence: nothing of the ViT's backward in the skipped steps
    cf, cs = _counts(full["lines"]), _counts(skip["lines"])
    print(f"[groups] launches per {STEPS} steps, full backward {cf}\n[groups] launches per {STEPS} steps, skipped       {cs}")
    vL = sa.vL
    assert cf["mic_vit_assemble_bwd"] == STEPS and cs["mic_vit_assemble_bwd"] == 0
    attn = ("mic_attn_bwd", "mic_attn_bwd_packed", "mic_attn_bwd_packed_tiled")
    assert sum(cf[k] for k in attn) - sum(cs[k] for k in attn) == STEPS * vL          # one attention backward per ViT layer
    ln = ("mic_layernorm_bwd", "mic_layernorm_bwd_partials")
    assert sum(cf[k] for k in ln) - sum(cs[k] for k in ln) == STEPS * (2 * vL + 1)    # two LayerNorms per layer and the pre-LayerNorm
    # plain GEMMs: per layer the dX of fc2, fc1, o, qkv; the bridge's dX; the patch-embedding dW
    assert cf["mic_gemm"] - cs["mic_gemm"] == STEPS * (4 * vL + 2), (cf["mic_gemm"], cs["mic_gemm"])
    assert cf["mic_gemm_grouped"] > cs["mic_gemm_grouped"]                            # the layers' weight-gradient launches
    # the grouped optimizer ran in both, and the plain entry points in neither
    for run in (full, skip):
        names = {_name(ln_) for ln_ in run["lines"]}
        assert "mic_adamw_groups" in names and not names & {"mic_adamw", "mic_adamw_rows", "mic_adamw_acc", "mic_adamw_clip"}


def test_grouped_step_with_the_optimizer_in_one_launch(dev):
    """overlap_optimizer=False: the serial whole-buffer path goes through the grouped kernel too — one launch per step over the whole
    buffer — with the frozen bytes intact and every leaf within the same 2e-5 of the oracle stepped per leaf"""
    from mic_amd.params import flatten_tree

    a = _run(dev, torch.float32, trace=True, param_groups=_groups(), overlap_optimizer=False)
    names = [_name(ln) for ln in a["lines"]]
    assert names.count("mic_adamw_groups") == STEPS and a["tr"].reducer.on_ready is None
    sa = a["model"].store
    for (x, y, _, _, f) in a["tr"]._group_runs:
        if f:
            assert torch.equal(_bits(sa.master[x:y]), _bits(a["first"]["master"][x:y])) and not sa.m[x:y].any() and not sa.v[x:y].any()
    ref, _, _ = _oracle_steps(a["rc"], a["p"], _leaf_groups(sa, _groups(), WD))
    got = flatten_tree(a["model"].params)
    dist = {k: (torch.from_numpy(got[k]) - rv).abs().max().item() for k, rv in ref.items()}
    print(f"[groups] one-launch grouped oracle: worst {max(dist.values()):.3e} (bound 2e-5)")
    assert all(d < 2e-5 for d in dist.values()), sorted(dist.items(), key=lambda kv: -kv[1])[:5]
