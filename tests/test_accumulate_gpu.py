"""Gradient accumulation: `Trainer(accumulate_steps=N)` on one GPU performs the optimizer step of an N-rank data-parallel run
(`lax.pmean(grad)` over N devices, then one AdamW step: main.py:698-701), up to fp32 summation order — checked against the oracle
with the tolerances the data-parallel and the single-step tests use (tests/test_ddp_gpu.py, tests/test_model_gpu.py).

The micro-batches come from different seeds, so their decoder ids differ: embedding rows that only an EARLIER micro-batch touches
are not flagged on the last micro-step, and their gradient has to arrive through the running sum."""
import os
import sys

import numpy as np
import pytest
import torch

from util_small import batch, make_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 2, 12
SIZES = [4, 4100, 8192 * 256 * 4 + 4 * 1031]  # one float4; a few blocks with a ragged last one; one full grid (8192 x 256 float4) + a remainder
OFF = 12                                      # start of the slice inside the larger buffer: non-zero, 16-byte aligned


def _b(shard):
    px, labels, mask, dec_in = shard
    return {"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}


_ORACLE = {}


def _oracle(rc, p, seed):
    """(shard, loss, grads) of the oracle on the micro-batch of `seed` at the INITIAL parameters: computed once, shared, never modified"""
    from oracle import train_ref

    if seed not in _ORACLE:
        sh = batch(rc, B, T, seed=seed, ragged=True)
        l, g = train_ref.loss_and_grads(rc, p, *sh)
        _ORACLE[seed] = (sh, l.item(), g)
    return _ORACLE[seed]


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", SIZES)
def test_grad_accumulate_is_bitwise_torch(dev, n):
    from mic_amd import ops

    g = torch.Generator(device=dev).manual_seed(n)
    total = OFF + n + 64
    src_buf = torch.randn(total, device=dev, generator=g)
    dst_buf = torch.randn(total, device=dev, generator=g)
    for init in (True, False):
        dst, want = dst_buf.clone(), dst_buf.clone()
        want[OFF:OFF + n] = src_buf[OFF:OFF + n] if init else dst_buf[OFF:OFF + n] + src_buf[OFF:OFF + n]
        assert dst[OFF:].data_ptr() % 16 == 0
        ops.grad_accumulate(dst[OFF:OFF + n], src_buf[OFF:OFF + n], init=init)
        torch.cuda.synchronize()
        assert torch.equal(dst, want), (init, n)  # the slice bit for bit, everything outside it untouched
    # the default length is the destination's; an explicit one is honoured
    dst = dst_buf.clone()
    ops.grad_accumulate(dst[OFF:], src_buf[OFF:], init=False, n=n)
    want = dst_buf.clone()
    want[OFF:OFF + n] += src_buf[OFF:OFF + n]
    torch.cuda.synchronize()
    assert torch.equal(dst, want)


def test_grad_accumulate_refuses_a_length_that_is_no_multiple_of_4(dev):
    from mic_amd import _lib, ops

    a, b = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    for n in (1, 6, 63):
        with pytest.raises(_lib.MicError):
            ops.grad_accumulate(a, b, n=n)
    torch.cuda.synchronize()
    assert not a.any()


def _adamw_state(dev, n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda s: torch.randn(n, device=dev, generator=g) * s
    return dict(p=r(0.02), m=r(1e-3), v=r(1e-3).square(), g=r(1e-2), acc=r(2e-2))


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("n", SIZES)
def test_adamw_acc_is_bitwise_adamw_on_the_summed_gradient(dev, n, t):
    from mic_amd import ops

    s = _adamw_state(dev, n, 1000 + n)
    hyper = torch.tensor([1e-3, float(t)], device=dev)
    gsum = s["g"] + s["acc"]  # one IEEE fp32 add per element, rounded before grad_scale is applied
    res = []
    for fused in (False, True):
        p, m, v = s["p"].clone(), s["m"].clone(), s["v"].clone()
        lp = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        ops.adamw(p, m, v, s["g"] if fused else gsum, lp, hyper, 0.9, 0.999, 1e-8, 0.01, grad_scale=1.0 / 3.0,
                  acc=s["acc"] if fused else None)
        res.append((p, m, v, lp))
    torch.cuda.synchronize()
    for name, a, b in zip("p m v p_lp".split(), *res):
        assert torch.equal(a, b), (name, n, t, (a.float() - b.float()).abs().max().item())
    assert not torch.equal(res[0][0], s["p"])  # (the update did something)


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("rows", [1, 37, 8192 * 8 + 13])  # one row; a few blocks; more rows than the grid has blocks
def test_adamw_rows_acc_is_bitwise_adamw_rows_on_the_summed_gradient(dev, rows, t):
    from mic_amd import ops

    width = 128
    n = rows * width
    s = _adamw_state(dev, n, 2000 + rows)
    hyper = torch.tensor([1e-3, float(t)], device=dev)
    flags = (torch.rand(rows, device=dev, generator=torch.Generator(device=dev).manual_seed(rows)) < 0.4).to(torch.uint8)
    gsum = s["g"] + s["acc"]
    for want in (0, 1):
        res = []
        for fused in (False, True):
            p, m, v = s["p"].clone(), s["m"].clone(), s["v"].clone()
            lp = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            ops.adamw_rows(rows, width, flags, want, p, m, v, s["g"] if fused else gsum, lp, hyper, 0.9, 0.999, 1e-8, 0.01,
                           grad_scale=1.0 / 3.0, acc=s["acc"] if fused else None)
            res.append((p, m, v, lp))
        torch.cuda.synchronize()
        for name, a, b in zip("p m v p_lp".split(), *res):
            assert torch.equal(a, b), (name, rows, t, want)
        skip = (flags != 0) != bool(want)  # rows the pass must leave alone
        p, m, v, lp = (x.view(rows, width) for x in res[1])
        assert torch.equal(p[skip], s["p"].view(rows, width)[skip]) and torch.equal(m[skip], s["m"].view(rows, width)[skip])
        assert torch.equal(v[skip], s["v"].view(rows, width)[skip]) and not lp[skip].any()
        if (~skip).any():
            assert not torch.equal(p[~skip], s["p"].view(rows, width)[~skip])


# ---------------------------------------------------------------------------------------------------------------- one process
def _accumulated_step_against_oracle(dev, N, dtype=torch.float32, **trainer_kw):
    """one optimizer step over N micro-batches (seeds 500 .. 500 + N - 1) against the oracle's mean gradient and its AdamW step"""
    from mic_amd import Trainer, create_learning_rate_fn
    from mic_amd.params import flatten_tree
    from oracle import train_ref

    fp32 = dtype == torch.float32
    rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    tr = Trainer(model, create_learning_rate_fn(40, 4, 1, 0, 1e-3), weight_decay=0.01, seed=42, bucket_mb=0.25, accumulate_steps=N,
                 **trainer_kw)
    assert len(tr.buckets) > 3 and model.store.acc is not None
    ref = [_oracle(rc, p, 500 + j) for j in range(N)]
    ids = [set(sh[3].reshape(-1).tolist()) for (sh, _, _) in ref]
    assert set().union(*ids[:-1]) - ids[-1], "some embedding rows must be touched by an earlier micro-batch only"
    master0 = model.store.master.clone()
    init = {k: v.copy() for k, v in flatten_tree(model.params).items()}
    for j in range(N - 1):
        out = tr.train_step(_b(ref[j][0]))
        torch.cuda.synchronize()
        assert tr.step == 0
        assert torch.equal(model.store.master, master0), "a micro-step that only accumulates must leave the weights alone"
        now = flatten_tree(model.params)
        assert all(np.array_equal(now[k], init[k]) for k in init)
        assert abs(float(out["loss"]) - ref[j][1]) < (5e-5 if fp32 else 2e-2) * max(1.0, abs(ref[j][1]))  # its own micro-batch's loss
        assert abs(float(out["learning_rate"]) - 1e-3) < 1e-9                                              # the pending step's
    out = tr.train_step(_b(ref[N - 1][0]))
    torch.cuda.synchronize()
    assert tr.step == 1
    mean_loss = sum(l for (_, l, _) in ref) / N
    print(f"[accumulate N={N} {dtype}] loss {float(out['loss']):.6f} vs oracle mean {mean_loss:.6f}")
    if fp32:
        assert abs(float(out["loss"]) - mean_loss) < 5e-5, (float(out["loss"]), mean_loss)
    else:
        assert abs(float(out["loss"]) - mean_loss) < 2e-2 * max(1.0, abs(mean_loss)), (float(out["loss"]), mean_loss)
    assert abs(float(out["learning_rate"]) - 1e-3) < 1e-9
    gm = {k: sum(g[k] for (_, _, g) in ref) / N for k in p}
    g_last, g_acc = model.store.export_flat("grad"), model.store.export_flat("acc")
    got = flatten_tree(model.params)
    worst, checked = {}, set()
    for k in p:
        mine = (torch.from_numpy(g_last[k]) + torch.from_numpy(g_acc[k])).reshape(gm[k].shape) / N
        sc = gm[k].abs().max().item()
        if sc > 1e-6:
            worst[k] = ((mine - gm[k]).abs().max() / sc).item()
            checked.add(k)
        else:  # analytically zero (post_layernorm, the attention k_proj biases): fp noise on both sides
            assert mine.abs().max().item() < (1e-6 if fp32 else 2e-3), (k, mine.abs().max().item())
        if fp32:
            newp, _, _ = train_ref.adamw_update(p[k], gm[k], torch.zeros_like(p[k]), torch.zeros_like(p[k]), 0, 1e-3, wd=0.01)
            d = (torch.from_numpy(got[k]).reshape(newp.shape) - newp).abs().max().item()
            assert d < 1e-4, (k, d)
    print(f"[accumulate N={N} {dtype}] worst gradient errors (of scale): {sorted(worst.items(), key=lambda kv: -kv[1])[:3]}")
    assert "model/shared/embedding" in checked
    bad = {k: v for k, v in worst.items() if v > (5e-4 if fp32 else 8e-2)}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    if not fp32:
        a = torch.cat([(torch.from_numpy(g_last[k]) + torch.from_numpy(g_acc[k])).reshape(-1) / N for k in p])
        b = torch.cat([gm[k].reshape(-1) for k in p])
        c = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
        print(f"[accumulate N={N} {dtype}] cosine {c:.6f}")
        assert c > 0.995, c
    return tr


@pytest.mark.parametrize("N", [2, 3])
def test_accumulated_step_matches_oracle_mean_gradient_step(dev, N):
    tr = _accumulated_step_against_oracle(dev, N)
    assert tr.overlap_optimizer and tr._split_shared  # per-bucket passes, the tied embedding's rows split: the default path


def test_accumulated_step_with_the_optimizer_in_one_launch(dev):
    tr = _accumulated_step_against_oracle(dev, 2, overlap_optimizer=False)
    assert not tr.overlap_optimizer and tr.reducer.on_ready is None


def test_accumulated_step_bf16_packed_rows(dev):
    """the benchmarked configuration in small (bf16 storage, packed decoder rows, compact head), against the fp32 oracle with the
    bounds one bf16 step is held to (tests/test_model_gpu.py::test_loss_and_grads_match_oracle)"""
    tr = _accumulated_step_against_oracle(dev, 2, dtype=torch.bfloat16)
    assert tr._pack is not None and tr.compact_head


def test_two_accumulated_steps_match_oracle_adamw(dev):
    """two optimizer steps of N = 2 under a warm-up schedule against the oracle's two AdamW steps on the two mean gradients: the
    second accumulation must START from its first micro-batch's gradient, not from the first accumulation's sum"""
    from mic_amd import Trainer, create_learning_rate_fn
    from mic_amd.params import flatten_tree
    from oracle import train_ref

    N = 2
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    lr_fn = create_learning_rate_fn(train_ds_size=40, train_batch_size=4, num_train_epochs=1, num_warmup_steps=2, learning_rate=1e-3)
    tr = Trainer(model, lr_fn, weight_decay=0.01, seed=42, bucket_mb=0.25, accumulate_steps=N)
    params = {k: v.clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(v) for k, v in p.items()}
    for step in range(2):
        lr = train_ref.linear_warmup_decay(step, 1e-3, 2, 10)
        losses, grads = [], []
        for j in range(N):
            seed = 500 + N * step + j
            if step == 0:
                sh, l, g = _oracle(rc, p, seed)
            else:
                sh = batch(rc, B, T, seed=seed, ragged=True)
                l, g = train_ref.loss_and_grads(rc, params, *sh)
                l = l.item()
            out = tr.train_step(_b(sh))
            losses.append(l)
            grads.append(g)
            assert abs(float(out["learning_rate"]) - lr) < 1e-9, (step, j, float(out["learning_rate"]), lr)
            assert tr.step == step + (1 if j == N - 1 else 0)
        assert abs(float(out["loss"]) - sum(losses) / N) < 5e-5 * max(1.0, sum(losses) / N)
        for k in params:
            params[k], m[k], v[k] = train_ref.adamw_update(params[k], sum(g[k] for g in grads) / N, m[k], v[k], step, lr, wd=0.01)
    gf = flatten_tree(model.params)
    worst = max(((torch.from_numpy(gf[k]).reshape(rv.shape) - rv).abs().max().item(), k) for k, rv in params.items())
    print(f"[two accumulated steps] largest parameter difference {worst}")
    assert worst[0] < 2e-5, worst


def test_accumulate_steps_1_is_the_default_trainer(dev):
    """`accumulate_steps=1` against a Trainer built without the keyword, identical models, two steps on the same batches.  The two
    runs issue the same launches, so they can differ only by the run-to-run noise of the atomically accumulated gradients (bias /
    LayerNorm / embedding rows; tests/test_model_gpu.py::test_split_embedding_adamw_and_masked_optimizer_stream_change_nothing): the
    same losses to 1e-5, weights within 2.5 lr per step and all but a sliver within 1e-6.  The moments are linear (m) and quadratic (v)
    in gradients whose atomic sums of a few dozen fp32 terms differ by ~1e-6 of their scale: within 1e-3 of the buffer's largest entry
    — a gradient counted twice or scaled by another factor moves them by O(1) of it."""
    from mic_amd import Trainer, create_learning_rate_fn

    lr, steps, res = 1e-3, 2, {}
    for mode, kw in (("default", {}), ("one", dict(accumulate_steps=1))):
        rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 0, lr), weight_decay=0.01, bucket_mb=0.25, **kw)
        losses = [float(tr.train_step(_b(batch(rc, B, T, seed=90 + s)))["loss"]) for s in range(steps)]
        torch.cuda.synchronize()
        assert tr.step == steps and model.store.acc is None, "the running-sum buffer must not exist without accumulation"
        res[mode] = (losses, model.store.master.clone(), model.store.m.clone(), model.store.v.clone())
    assert np.allclose(res["one"][0], res["default"][0], rtol=1e-5), (res["one"][0], res["default"][0])
    diff = (res["one"][1] - res["default"][1]).abs()
    assert diff.max().item() <= 2.5 * lr * steps, diff.max().item()
    assert (diff > 1e-6).float().mean().item() < 1e-3, (diff > 1e-6).float().mean().item()
    for i, name in ((2, "m"), (3, "v")):
        d = (res["one"][i] - res["default"][i]).abs().max().item()
        assert d <= 1e-3 * res["default"][i].abs().max().item(), (name, d)


def test_out_of_scope_combinations_and_mid_accumulation_checkpoint(dev, tmp_path):
    from mic_amd import Trainer, create_learning_rate_fn

    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    lr_fn = create_learning_rate_fn(40, 4, 1, 0, 1e-3)
    with pytest.raises(ValueError, match="fp8"):
        Trainer(model, lr_fn, accumulate_steps=2, gemm_dtype="fp8")
    assert not model.engine.fp8  # refused before anything was switched
    with pytest.raises(ValueError, match="emulate_comm"):
        Trainer(model, lr_fn, accumulate_steps=2, emulate_comm=8)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="accumulate_steps"):
            Trainer(model, lr_fn, accumulate_steps=bad)
    tr = Trainer(model, lr_fn, accumulate_steps=2, bucket_mb=0.25)
    b = _b(batch(rc, B, T, seed=500))
    tr.train_step(b)
    with pytest.raises(RuntimeError, match="accumulation"):
        tr.save_checkpoint(str(tmp_path), with_opt=True)
    assert not os.listdir(str(tmp_path))
    tr.train_step(b)
    ckpt = tr.save_checkpoint(str(tmp_path), with_opt=True)  # after the optimizer step: as without accumulation
    assert tr.step == 1 and os.path.isdir(ckpt)
    tr.train_step(b)
    assert tr._micro == 1
    assert tr.restore_checkpoint(ckpt) == 1 and tr._micro == 0  # the pending accumulation belonged to the replaced state
    out = tr.train_step(b)
    assert tr._micro == 1 and tr.step == 1 and np.isfinite(float(out["loss"]))


# ---------------------------------------------------------------------------------------------------------------- two processes
def _worker(rank, world, port, q):
    """(a) world 2 x N = 2, fp32, no dropout: the step of a 4-rank run.  (b) dropout 0.1: one process x N = 2 draws the masks of the
    two ranks of a plain two-rank step on the same two shards (the virtual-rank dropout streams)."""
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        _worker_body(rank, world, q)
    except Exception as ex:  # the parent must hear of a failure instead of waiting for its queue
        import traceback

        q.put((rank, False, f"{ex!r}\n{traceback.format_exc()}"))


def _worker_body(rank, world, q):
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    try:
        import mic_amd  # noqa: F401
        from mic_amd import Trainer, create_learning_rate_fn
        from mic_amd.params import flatten_tree
        from oracle import train_ref

        ok, msg = True, ""
        N = 2
        lr_fn = create_learning_rate_fn(40, 4, 1, 0, 1e-3)
        # ---- (a)
        rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
        tr = Trainer(model, lr_fn, weight_decay=0.01, seed=42, bucket_mb=0.25, accumulate_steps=N)
        assert len(tr.buckets) > 3 and tr.world == 2
        shards = [batch(rc, B, T, seed=500 + k, ragged=True) for k in range(world * N)]  # shard of virtual rank r * N + j
        master0 = model.store.master.clone()
        out = tr.train_step(_b(shards[rank * N]))
        torch.cuda.synchronize()
        if tr.step != 0 or not torch.equal(model.store.master, master0):
            ok, msg = False, "the accumulating micro-step changed the state"
        out = tr.train_step(_b(shards[rank * N + 1]))
        torch.cuda.synchronize()
        w = model.store.master.cpu()
        ws = [torch.empty_like(w) for _ in range(world)]
        dist.all_gather(ws, w)
        if not all(torch.equal(ws[0], x) for x in ws):
            ok, msg = False, f"the ranks' parameters differ by {max(float((ws[0] - x).abs().max()) for x in ws)}"
        if tr.step != 1:
            ok, msg = False, f"step {tr.step}"
        if rank == 0 and ok:
            ref = [train_ref.loss_and_grads(rc, p, *sh) for sh in shards]
            mean_loss = sum(l.item() for l, _ in ref) / len(ref)
            if abs(float(out["loss"]) - mean_loss) > 5e-5:
                ok, msg = False, f"loss {float(out['loss'])} vs {mean_loss}"
            gsum = model.store.export_flat("grad")  # the all-reduced g + acc of both ranks: the SUM over the four shards
            got = flatten_tree(model.params)
            for k in p:
                gm = sum(g[k] for _, g in ref) / len(ref)
                sc = gm.abs().max().item()
                if sc > 1e-6:
                    e = ((torch.from_numpy(gsum[k]).reshape(gm.shape) / len(ref) - gm).abs().max() / sc).item()
                    if e > 5e-4:
                        ok, msg = False, f"(a) grad {k}: {e}"
                        break
                newp, _, _ = train_ref.adamw_update(p[k], gm, torch.zeros_like(p[k]), torch.zeros_like(p[k]), 0, 1e-3, wd=0.01)
                d = (torch.from_numpy(got[k]).reshape(newp.shape) - newp).abs().max().item()
                if d > 1e-4:
                    ok, msg = False, f"(a) param {k}: {d}"
                    break
        del tr, model
        # ---- (b) the plain two-rank step with dropout, one micro-batch per rank ...
        rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        tr = Trainer(model, lr_fn, weight_decay=0.01, seed=42, bucket_mb=0.25)
        tr.train_step(_b(shards[rank]))
        torch.cuda.synchronize()
        two_rank = model.store.export_flat("grad")
        del tr, model
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    if rank == 0 and ok:
        # ... and, with the process group gone (world 1), the same two shards as the two micro-steps of ONE process
        rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        tr = Trainer(model, lr_fn, weight_decay=0.01, seed=42, bucket_mb=0.25, accumulate_steps=N)
        assert tr.world == 1
        for j in range(N):
            tr.train_step(_b(shards[j]))
        torch.cuda.synchronize()
        g_last, g_acc = model.store.export_flat("grad"), model.store.export_flat("acc")
        for k in two_rank:
            sc = np.abs(two_rank[k]).max()
            if sc > 1e-6:
                e = np.abs(g_last[k] + g_acc[k] - two_rank[k]).max() / sc
                if e > 5e-4:
                    ok, msg = False, f"(b) summed gradient {k}: {e} of scale (other dropout masks than the two ranks drew?)"
                    break
    q.put((rank, ok, msg))


def test_two_ranks_times_two_micro_steps_and_virtual_rank_dropout(dev):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 24100 + (os.getpid() % 2000)  # (tests/test_ddp_gpu.py draws from 29600 .. 32300)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for pr in procs:
        pr.join(timeout=60)
    assert all(r[1] for r in res), res
