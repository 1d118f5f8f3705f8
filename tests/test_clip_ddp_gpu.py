"""Global-norm clipping with several ranks: two processes on cuda:0 over gloo (the shape of tests/test_ddp_gpu.py), once plain and once
with accumulate_steps=2, max_grad_norm=1.0.  The norm is taken over the all-reduced buffer — the same bytes in a fixed order on every
rank — so `grad_norm` is bit-identical on both; rank 0 makes the assertions of tests/util_clip.py on the rank-mean gradient."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q, N):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    try:
        _worker_body(rank, world, q, N)
    except Exception as ex:  # the parent must hear of a failure instead of waiting for its queue
        import traceback

        q.put((rank, False, f"{ex!r}\n{traceback.format_exc()}"))


def _worker_body(rank, world, q, N):
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    try:
        import mic_amd  # noqa: F401
        from mic_amd import Trainer, create_learning_rate_fn
        from util_clip import B, T, as_batch, assert_oracle, assert_tight, oracle
        from util_small import batch, make_pair

        c = 1.0
        rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
        tr = Trainer(model, create_learning_rate_fn(40, 4, 1, 0, 1e-3), weight_decay=0.01, seed=42, bucket_mb=0.25, accumulate_steps=N,
                     max_grad_norm=c)
        assert len(tr.buckets) > 3 and tr.world == 2 and tr.reducer.on_ready is not None and not tr._split_shared
        shards = [batch(rc, B, T, seed=500 + k, ragged=True) for k in range(world * N)]  # shard of virtual rank r * N + j
        for j in range(N - 1):
            out = tr.train_step(as_batch(shards[rank * N + j]))
            assert "grad_norm" not in out and tr.step == 0
        out = tr.train_step(as_batch(shards[rank * N + N - 1]))
        torch.cuda.synchronize()
        assert tr.step == 1 and "grad_norm" in out
        bits = out["grad_norm"].reshape(1).view(torch.int32).cpu()
        both = [torch.empty_like(bits) for _ in range(world)]
        dist.all_gather(both, bits)
        ok, msg = True, ""
        if not all(torch.equal(both[0], x) for x in both):
            ok, msg = False, f"grad_norm differs between the ranks: bits {[int(x) for x in both]}"
        w = model.store.master.cpu()
        ws = [torch.empty_like(w) for _ in range(world)]
        dist.all_gather(ws, w)
        if not all(torch.equal(ws[0], x) for x in ws):
            ok, msg = False, f"the ranks' parameters differ by {max(float((ws[0] - x).abs().max()) for x in ws)}"
        if rank == 0 and ok:
            # the flat buffer holds the SUM over ranks (and micro-steps: acc joined g in front of the all-reduce); gscale = 1 / (world * N)
            assert abs(tr._gscale - 1.0 / (world * N)) < 1e-12
            assert_tight(tr, out, c, with_acc=False, tag=f" ddp N={N}")
            ref = [oracle(rc, p, 500 + k) for k in range(world * N)]
            gm = {k: sum(g[k] for (_, _, g) in ref) / len(ref) for k in p}
            assert_oracle(tr, out, p, gm, c, True, tag=f" ddp N={N}")
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()
    q.put((rank, ok, msg))


@pytest.mark.parametrize("N", [1, 2])
def test_two_rank_clipped_step(dev, N):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 26500 + (os.getpid() % 2000) + 2000 * (N - 1) // 4  # (tests/test_ddp_gpu.py: 29600 .. 32300, test_accumulate_gpu.py: 24100 .. 26100)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, N)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for pr in procs:
        pr.join(timeout=60)
    assert all(r[1] for r in res), res
