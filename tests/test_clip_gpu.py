"""Global-norm gradient clipping: `Trainer(max_grad_norm=c)` = optax.chain(clip_by_global_norm(c), adamw(...)) on the gradient AdamW
consumes, and the kernels of csrc/optimizer.hip it is made of.

The first Adam step is lr * g / (|g| + eps) and Adam is invariant under a common scale of the gradient, so the weights alone cannot
show that clipping happened: the decisive observables are the returned norm and the moments m, v (tests/util_clip.py::assert_tight),
both checked against the model's own stored gradient at bounds derived from the arithmetic, not tuned.

Measured on the MI355X (see profiles/NOTES_r10.md for the run): the distance of `grad_norm` from the oracle's norm is printed by every
Trainer test ("[clip ...] grad_norm ... vs oracle")."""
import math

import numpy as np
import pytest
import torch

from util_clip import (B, B1, B2, T, as_batch, assert_oracle, assert_tight, clip_factor, norm64, oracle, sumsq_rel_bound)
from util_small import batch, make_pair

pytestmark = pytest.mark.gpu
OFF = 12  # start of every slice inside its larger buffer: non-zero, 16-byte aligned
NAN = float("nan")


def _sizes():
    """one float4; a few blocks with a ragged last one; one full grid of the sum of squares (its block cap x 256 float4) + a remainder"""
    from mic_amd import ops

    cap = ops.grad_sumsq_slots(1 << 40)
    full = cap * 256 * 4
    assert ops.grad_sumsq_slots(full) == cap and ops.grad_sumsq_slots(full - 1024) == cap - 1
    return [4, 4100, full + 4 * 1031]


SIZES = [0, 1, 2]  # indices into _sizes() (the sizes themselves come from the library's launch geometry)


def _rand(dev, n, seed, scale=1.0):
    return torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)) * scale


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_grad_sumsq_against_fp64_of_the_same_fp32_values(dev, size, with_acc):
    from mic_amd import ops

    n = _sizes()[size]
    slots = ops.grad_sumsq_slots(n)
    total = OFF + n + 64
    g_buf, a_buf = _rand(dev, total, 10 + n, 1e-2), _rand(dev, total, 20 + n, 2e-2)
    g0, a0 = g_buf.clone(), a_buf.clone()
    g, acc = g_buf[OFF:OFF + n], (a_buf[OFF:OFF + n] if with_acc else None)
    assert g.data_ptr() % 16 == 0
    x = (g + acc) if with_acc else g  # one IEEE fp32 add per element: the term the kernel squares
    want = float((x.double() ** 2).sum())
    parts = [torch.full((slots + 8,), NAN, device=dev) for _ in range(2)]  # poisoned: nothing may rely on what the buffer held
    for pt in parts:
        assert ops.grad_sumsq(g, pt[3:], acc=acc, n=n) == slots
    torch.cuda.synchronize()
    got = float(parts[0][3:3 + slots].double().sum())
    bound = 2.0 * sumsq_rel_bound(n, slots)
    rel = abs(got - want) / want
    print(f"[grad_sumsq n={n} acc={with_acc}] {slots} slots, relative error {rel:.3e} (bound {bound:.3e})")
    assert rel <= bound, (got, want, rel, bound)
    assert torch.isnan(parts[0][:3]).all() and torch.isnan(parts[0][3 + slots:]).all(), "slots outside the written range were touched"
    assert torch.isfinite(parts[0][3:3 + slots]).all()
    assert torch.equal(g_buf, g0) and torch.equal(a_buf, a0), "inputs must stay untouched"
    assert torch.equal(parts[0][3:3 + slots].view(torch.int32), parts[1][3:3 + slots].view(torch.int32)), "same bytes, same bits"
    # the default length is the gradient's; the finaliser over these slots gives the norm (c = inf: measures, coefficient = grad_scale)
    out2 = torch.full((2,), NAN, device=dev)
    ops.clip_coef(parts[0][3:], slots, 0.25, math.inf, out2)
    pt = torch.full((slots,), NAN, device=dev)
    ops.grad_sumsq(g, pt, acc=acc)
    torch.cuda.synchronize()
    assert torch.equal(pt.view(torch.int32), parts[0][3:3 + slots].view(torch.int32))
    norm = 0.25 * math.sqrt(want)
    assert abs(float(out2[0]) - norm) <= bound * norm and float(out2[1]) == 0.25


def _coef(dev, g, gscale, c):
    from mic_amd import ops

    g = torch.tensor(g, dtype=torch.float32, device=dev)
    parts = torch.full((ops.grad_sumsq_slots(g.numel()),), NAN, device=dev)
    out2 = torch.full((2,), NAN, device=dev)
    ops.clip_coef(parts, ops.grad_sumsq(g, parts), gscale, c, out2)
    torch.cuda.synchronize()
    return float(out2[0]), float(out2[1])


@pytest.mark.parametrize("c,coef", [(2.0, 0.4), (2.5, 0.5), (3.0, 0.5), (math.inf, 0.5)])
def test_clip_coef_known_answers(dev, c, coef):
    """g = [3, 4, 0, 0], gscale = 0.5: the norm is exactly 2.5.  c = 2.5 does NOT satisfy optax's strict `norm < c` — the second branch
    gives 0.5 * 2.5 / 2.5 = 0.5 all the same"""
    norm, got = _coef(dev, [3.0, 4.0, 0.0, 0.0], 0.5, c)
    assert norm == 2.5
    assert abs(got - coef) <= 2.0 ** -23 * coef, (got, coef)
    if c >= 2.5:
        assert got == 0.5


def test_clip_coef_zero_and_infinite_norms(dev):
    """no special cases: IEEE arithmetic gives what optax's where(trigger, t, t / g_norm * max_norm) gives"""
    assert _coef(dev, [0.0] * 8, 0.5, 1.0) == (0.0, 0.5)          # a zero norm triggers the first branch; no NaN
    assert _coef(dev, [1.0, math.inf, 0.0, 2.0], 0.5, 1.0) == (math.inf, 0.0)
    assert _coef(dev, [0.0, 0.0, 2e19, 0.0], 0.5, 1.0) == (math.inf, 0.0)  # the fp32 square overflows, as an fp32 computation does
    norm, coef = _coef(dev, [1.0, NAN, 0.0, 2.0], 0.5, 1.0)
    assert math.isnan(norm) and math.isnan(coef)


def _adamw_state(dev, total, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda s: torch.randn(total, device=dev, generator=g) * s
    return dict(p=r(0.02), m=r(1e-3), v=r(1e-3).square(), g=r(1e-2), acc=r(2e-2))


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("with_acc", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_adamw_clip_is_bitwise_adamw_at_the_coefficient_read_back(dev, size, with_acc, t):
    from mic_amd import ops

    n = _sizes()[size]
    total = OFF + n + 64
    s = _adamw_state(dev, total, 3000 + n)
    sl = slice(OFF, OFF + n)
    acc = s["acc"][sl] if with_acc else None
    hyper = torch.tensor([1e-3, float(t)], device=dev)
    parts = torch.full((ops.grad_sumsq_slots(n),), NAN, device=dev)
    out2 = torch.full((2,), NAN, device=dev)
    ops.clip_coef(parts, ops.grad_sumsq(s["g"][sl], parts, acc=acc), 1.0 / 3.0, 1e-3, out2)  # (norm ~ 1e-2 sqrt(n) / 3: clips)
    torch.cuda.synchronize()
    coef = float(out2[1])  # the fp32 coefficient as a host float
    assert 0.0 < coef < float(np.float32(1.0 / 3.0))
    res = []
    for clip in (False, True):
        p, m, v = s["p"].clone(), s["m"].clone(), s["v"].clone()
        lp = torch.zeros(total, dtype=torch.bfloat16, device=dev)
        if clip:
            ops.adamw_clip(p[sl], m[sl], v[sl], s["g"][sl], lp[sl], hyper, out2[1:], B1, B2, 1e-8, 0.01, acc=acc)
        else:
            ops.adamw(p[sl], m[sl], v[sl], s["g"][sl], lp[sl], hyper, B1, B2, 1e-8, 0.01, grad_scale=coef, acc=acc)
        res.append((p, m, v, lp))
    torch.cuda.synchronize()
    for name, a, b in zip("p m v p_lp".split(), *res):
        assert torch.equal(a, b), (name, n, t, with_acc)  # the slice bit for bit, everything outside it untouched alike
    assert not torch.equal(res[1][0][sl], s["p"][sl]) and torch.equal(res[1][0][:OFF], s["p"][:OFF]) and torch.equal(res[1][0][OFF + n:], s["p"][OFF + n:])


def test_refused_calls_write_nothing(dev):
    from mic_amd import _lib, ops

    g, acc = torch.ones(64, device=dev), torch.ones(64, device=dev)
    parts = torch.full((8,), NAN, device=dev)
    out2 = torch.full((2,), NAN, device=dev)
    p, m, v = torch.zeros(64, device=dev), torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    lp = torch.zeros(64, dtype=torch.bfloat16, device=dev)
    hyper, coef = torch.tensor([1e-3, 1.0], device=dev), torch.ones(1, device=dev)
    for n in (1, 6, 63):  # no multiple of 4
        with pytest.raises(_lib.MicError):
            ops.grad_sumsq(g, parts, n=n)
        with pytest.raises(_lib.MicError):
            ops.adamw_clip(p, m, v, g, lp, hyper, coef, B1, B2, 1e-8, 0.01, n=n)
    with pytest.raises(_lib.MicError):  # a slice that starts 4 bytes behind a 16-byte boundary
        ops.grad_sumsq(g[1:9], parts, n=8)
    with pytest.raises(_lib.MicError):
        ops.grad_sumsq(g[:8], parts, acc=acc[1:9], n=8)
    for bad in ("p", "m", "v", "g", "acc"):
        a = dict(p=p[:8], m=m[:8], v=v[:8], g=g[:8], acc=acc[:8])
        a[bad] = dict(p=p, m=m, v=v, g=g, acc=acc)[bad][1:9]
        with pytest.raises(_lib.MicError):
            ops.adamw_clip(a["p"], a["m"], a["v"], a["g"], lp[:8], hyper, coef, B1, B2, 1e-8, 0.01, acc=a["acc"])
    with pytest.raises(_lib.MicError):  # no slots
        ops.clip_coef(torch.ones(8, device=dev), 0, 1.0, 1.0, out2)
    torch.cuda.synchronize()
    assert torch.isnan(parts).all() and torch.isnan(out2).all()
    assert not p.any() and not m.any() and not v.any() and not lp.any()


# ---------------------------------------------------------------------------------------------------------------- Trainer
LR = 1e-3


def _clipped_step(dev, c, N=1, dtype=torch.float32, before_step=None, tag="", **trainer_kw):
    """one optimizer step over N micro-batches (seeds 500 .. 500 + N - 1) with max_grad_norm=c: the tight assertions against the model's
    own gradient and the oracle's clipped AdamW step.  Returns (trainer, step output, norm read back, coef, distance from the oracle)."""
    from mic_amd import Trainer, create_learning_rate_fn

    fp32 = dtype == torch.float32
    rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    tr = Trainer(model, create_learning_rate_fn(40, 4, 1, 0, LR), weight_decay=0.01, seed=42, bucket_mb=0.25, accumulate_steps=N,
                 max_grad_norm=c, **trainer_kw)
    assert len(tr.buckets) > 3 and not tr._split_shared and tr._clip_partials is not None
    ref = [oracle(rc, p, 500 + j) for j in range(N)]
    if before_step is not None:
        before_step(tr)
    for j in range(N - 1):
        out = tr.train_step(as_batch(ref[j][0]))
        assert "grad_norm" not in out and tr.step == 0, "a micro-step that only accumulates takes no optimizer step and reports no norm"
    out = tr.train_step(as_batch(ref[N - 1][0]))
    torch.cuda.synchronize()
    assert tr.step == 1 and set(out) == {"loss", "learning_rate", "grad_norm"}
    assert out["grad_norm"].is_cuda and out["grad_norm"].dim() == 0
    mean_loss = sum(l for (_, l, _) in ref) / N
    assert abs(float(out["loss"]) - mean_loss) < (5e-5 if fp32 else 2e-2) * max(1.0, abs(mean_loss))
    tag = f" {tag or ''} c={c} N={N} {str(dtype).split('.')[-1]}"
    norm, coef = assert_tight(tr, out, c, with_acc=N > 1, tag=tag)
    gm = {k: sum(g[k] for (_, _, g) in ref) / N for k in p}
    dist = assert_oracle(tr, out, p, gm, c, fp32, lr=LR, tag=tag)
    return tr, out, norm, coef, dist


def test_oracle_norms_sit_far_from_both_thresholds():
    """the norms the cases below rely on (fp64 of the oracle's gradients at the initial weights): 1.0 clips and 10.0 does not, each
    a factor >= 2.5 away — no case sits near the trigger"""
    rc, p, _ = _cpu_pair()
    norms = {s: norm64(oracle(rc, p, s)[2]) for s in (500, 501, 502)}
    g0, g1 = oracle(rc, p, 500)[2], oracle(rc, p, 501)[2]
    norms["mean"] = norm64({k: (g0[k] + g1[k]) / 2 for k in g0})
    print(f"[clip] oracle norms {norms}")
    for k, want in ((500, 3.4188), (501, 3.4213), (502, 3.8829), ("mean", 2.5216)):
        assert abs(norms[k] - want) < 5e-4, (k, norms[k], want)
        assert 2.5 * 1.0 <= norms[k] <= 10.0 / 2.5


def _cpu_pair():
    """the oracle's config and initial parameters alone (no product model, no device)"""
    from oracle import model_ref as M
    from util_small import SEED, ref_config

    rc = ref_config("tanh", 1e-6, dropout=0.0)
    return rc, M.init_params(rc, seed=SEED, perturb_ln=True), None


def test_clipping_scales_the_moments_fp32_default_path(dev):
    """c = 1.0 clips (norm 3.42): the first moment is 1 / norm ~ 0.29 of what c = 10.0 (no clipping) leaves, the second its square.
    The two runs' gradients differ only by the run-to-run noise of the atomically accumulated ones (~1e-6 of their scale)."""
    tr1, _, norm1, coef1, _ = _clipped_step(dev, 1.0)
    assert tr1.overlap_optimizer and tr1.reducer.on_ready is not None  # the sums of squares ran per bucket
    assert abs(coef1 - 1.0 / norm1) < 1e-6 and 0.28 < coef1 < 0.30
    m1, v1 = tr1.model.store.m.double().norm().item(), tr1.model.store.v.double().sum().item()
    tr10, _, norm10, coef10, _ = _clipped_step(dev, 10.0)
    assert coef10 == 1.0 and float(tr10._clip_out[1]) == 1.0  # not clipped: the coefficient is exactly gscale
    assert abs(norm10 - norm1) < 1e-5 * norm1
    m10, v10 = tr10.model.store.m.double().norm().item(), tr10.model.store.v.double().sum().item()
    assert abs(m1 / m10 - 1.0 / norm1) < 1e-4 / norm1, (m1 / m10, 1.0 / norm1)
    assert abs(v1 / v10 - 1.0 / norm1 ** 2) < 2e-4 / norm1 ** 2, (v1 / v10, 1.0 / norm1 ** 2)


def test_infinite_max_norm_measures_and_is_the_default_trainer(dev):
    """`max_grad_norm=inf` against a Trainer built without the keyword, identical models, two steps on the same batches, with the bounds
    of tests/test_accumulate_gpu.py::test_accumulate_steps_1_is_the_default_trainer (the two runs differ by the run-to-run noise of
    the atomically accumulated gradients only: the coefficient is exactly gscale, and adamw_clip is bitwise adamw at that scale)"""
    from mic_amd import Trainer, create_learning_rate_fn

    lr, steps, res = 1e-3, 2, {}
    for mode, kw in (("default", {}), ("inf", dict(max_grad_norm=math.inf))):
        rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 0, lr), weight_decay=0.01, bucket_mb=0.25, **kw)
        outs = [tr.train_step(as_batch(batch(rc, B, T, seed=90 + s))) for s in range(steps)]
        torch.cuda.synchronize()
        assert tr.step == steps
        if mode == "inf":
            assert all(math.isfinite(float(o["grad_norm"])) and float(o["grad_norm"]) > 0 for o in outs)
            assert float(tr._clip_out[1]) == 1.0
            assert outs[0]["grad_norm"].data_ptr() != outs[1]["grad_norm"].data_ptr()  # fresh storage per step
        else:
            assert all("grad_norm" not in o for o in outs)
        res[mode] = ([float(o["loss"]) for o in outs], model.store.master.clone(), model.store.m.clone(), model.store.v.clone())
    assert np.allclose(res["inf"][0], res["default"][0], rtol=1e-5), (res["inf"][0], res["default"][0])
    diff = (res["inf"][1] - res["default"][1]).abs()
    assert diff.max().item() <= 2.5 * lr * steps, diff.max().item()
    assert (diff > 1e-6).float().mean().item() < 1e-3, (diff > 1e-6).float().mean().item()
    for i, name in ((2, "m"), (3, "v")):
        d = (res["inf"][i] - res["default"][i]).abs().max().item()
        assert d <= 1e-3 * res["default"][i].abs().max().item(), (name, d)


def test_clipped_step_with_the_optimizer_in_one_launch(dev):
    tr, *_ = _clipped_step(dev, 1.0, overlap_optimizer=False, tag="one-launch")
    assert not tr.overlap_optimizer and tr.reducer.on_ready is None


def test_clipped_step_bf16_packed_rows(dev):
    tr, _, _, _, dist = _clipped_step(dev, 1.0, dtype=torch.bfloat16)
    assert tr._pack is not None and tr.compact_head


def test_clipped_accumulated_step(dev):
    """accumulate_steps=2, seeds 500 and 501: the norm is that of the MEAN gradient (~2.52), on fp32(g + acc)"""
    tr, out, norm, coef, _ = _clipped_step(dev, 1.0, N=2)
    assert abs(norm - 2.5216) < 5e-3 and tr.model.store.acc is not None
    tr, out, norm, coef, _ = _clipped_step(dev, 1.0, N=2, overlap_optimizer=False, tag="one-launch")
    assert abs(norm - 2.5216) < 5e-3


def test_two_clipped_steps_match_oracle_adamw_under_warmup(dev):
    """two optimizer steps under a warm-up schedule against the oracle's two AdamW steps with per-step clipping; the moment assertion
    after each step (the second against the first's moments)"""
    from mic_amd import Trainer, create_learning_rate_fn
    from mic_amd.params import flatten_tree
    from oracle import train_ref

    c = 1.0
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    lr_fn = create_learning_rate_fn(train_ds_size=40, train_batch_size=4, num_train_epochs=1, num_warmup_steps=2, learning_rate=1e-3)
    tr = Trainer(model, lr_fn, weight_decay=0.01, seed=42, bucket_mb=0.25, max_grad_norm=c)
    params = {k: v.clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(v) for k, v in p.items()}
    m_prev = v_prev = None
    for step in range(2):
        lr = train_ref.linear_warmup_decay(step, 1e-3, 2, 10)
        if step == 0:
            sh, l, g = oracle(rc, p, 500)
        else:
            sh = batch(rc, B, T, seed=501, ragged=True)
            l, g = train_ref.loss_and_grads(rc, params, *sh)
            l = l.item()
        out = tr.train_step(as_batch(sh))
        torch.cuda.synchronize()
        assert tr.step == step + 1 and abs(float(out["learning_rate"]) - lr) < 1e-9
        assert abs(float(out["loss"]) - l) < 5e-5 * max(1.0, abs(l))
        assert_tight(tr, out, c, with_acc=False, m_prev=m_prev, v_prev=v_prev, tag=f" two steps, step {step}")
        m_prev, v_prev = model.store.export_flat("m"), model.store.export_flat("v")
        n_ref = norm64(g)
        assert abs(float(out["grad_norm"]) - n_ref) <= 5e-4 * n_ref
        f = clip_factor(n_ref, c)
        for k in params:
            params[k], m[k], v[k] = train_ref.adamw_update(params[k], f * g[k], m[k], v[k], step, lr, wd=0.01)
    gf = flatten_tree(model.params)
    worst = max(((torch.from_numpy(gf[k]).reshape(rv.shape) - rv).abs().max().item(), k) for k, rv in params.items())
    print(f"[clip two steps] largest parameter difference {worst}")
    assert worst[0] < 2e-5, worst


def test_sums_of_squares_on_a_lagging_side_stream_are_waited_for(dev):
    """every per-bucket sum of squares sits behind a 2-ms spin on its side stream and the partials start as NaN: the finaliser (on the
    step's own stream) must still see every slot written — the tight assertions hold"""
    from mic_amd import ops

    calls = []

    def lag(tr):
        a, b = torch.zeros(1 << 18, device=dev), torch.zeros(1 << 18, device=dev)
        inner = tr._sumsq_slice

        def lagging(lo, hi):
            ops.comm_emulate(a, b, 1 << 20, 2000.0, 8)
            calls.append((lo, hi))
            return inner(lo, hi)
        tr._sumsq_slice = lagging
        tr._clip_partials.fill_(NAN)

    tr, *_ = _clipped_step(dev, 1.0, before_step=lag, tag="lagging")
    assert sorted(calls) == sorted(tr.buckets) and torch.isfinite(tr._clip_partials).all()


def test_out_of_scope_combinations_and_the_default_trainer(dev):
    from mic_amd import Trainer, create_learning_rate_fn

    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    lr_fn = create_learning_rate_fn(40, 4, 1, 0, 1e-3)
    with pytest.raises(ValueError, match="max_grad_norm.*fp8"):
        Trainer(model, lr_fn, max_grad_norm=1.0, gemm_dtype="fp8")
    assert not model.engine.fp8  # refused before anything was switched
    with pytest.raises(ValueError, match="max_grad_norm.*emulate_comm"):
        Trainer(model, lr_fn, max_grad_norm=1.0, emulate_comm=8)
    assert model.store.grad is None and model.store.m is None  # ... and before anything was allocated
    for bad in (True, NAN, 0.0, -1.0, "1"):
        with pytest.raises(ValueError, match="max_grad_norm"):
            Trainer(model, lr_fn, max_grad_norm=bad)
    tr = Trainer(model, lr_fn, bucket_mb=0.25)
    out = tr.train_step(as_batch(batch(rc, B, T, seed=500)))
    torch.cuda.synchronize()
    assert set(out) == {"loss", "learning_rate"} and tr._clip_partials is None and tr._clip_out is None and tr.max_grad_norm is None
    assert tr._split_shared  # the default path keeps the row split
