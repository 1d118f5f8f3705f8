"""Several captions per image in one train step (batch["captions_per_image"] = G, Engine passes with images=n_img) on the GPU.

The step must be the reference step on pixel_values.repeat_interleave(G, 0): every comparison here is against the oracle on the
repeated pixels, or against the product's own step fed the repeated pixels, under the bounds the existing suites apply to the plain
step (tests/test_model_gpu.py, tests/test_ddp_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from util_small import batch, make_pair  # noqa: E402

pytestmark = pytest.mark.gpu


def grouped(rc, n_img, G, T, seed):
    """n_img images and n_img * G ragged captions, image-major"""
    px = batch(rc, n_img, T, seed=seed)[0]
    _, labels, mask, dec_in = batch(rc, n_img * G, T, seed=seed + 1)
    return px, labels, mask, dec_in


def bdict(px, labels, mask, dec_in, G=None):
    b = {"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}
    if G is not None:
        b["captions_per_image"] = G
    return b


def oracle_masks(model, rc, seed, B, T):
    """the keep-masks of the fused dropout epilogues in the oracle's dict form (tests/test_model_gpu.py: _oracle_masks); the sites
    index caption rows, so B is the number of captions"""
    from mic_amd import ops
    from mic_amd.engine import _mix

    n = B * T * rc.d_model
    m = {"embed": ops.dropout_mask(n, rc.dropout, _mix(seed, 1), model.device).cpu().reshape(B, T, rc.d_model)}
    for l in range(rc.d_layers):
        for j, name in enumerate(("self", "cross", "ffn")):
            m[f"{l}/{name}"] = ops.dropout_mask(n, rc.dropout, _mix(seed, 10 + 3 * l + j), model.device).cpu().reshape(B, T, rc.d_model)
    return m


def engine_args(model, px, labels, mask, dec_in, *, compact, pack, G):
    """(positional args, keyword args) of Engine.loss_and_grads / loss_only for the batch; pack implies compact"""
    from mic_amd import group_packed_rows, loss_rows, packed_rows

    dev = model.device
    d = lambda x, t: model._dev(x, t)  # noqa: E731
    B, T = labels.shape
    kw = {}
    if compact or pack:
        idx, rl = loss_rows(mask.numpy(), labels.numpy())
        assert 0 < len(idx) < B * T
        kw = dict(rows=(d(idx, torch.int32), len(idx)), row_labels=d(rl, torch.int32))
    if pack:
        q_off, q_len, ids, pos = packed_rows(mask.numpy(), dec_in.numpy())
        extra = tuple(d(t, torch.int32) for t in group_packed_rows(q_off, q_len, G)) if G > 1 else ()
        kw["pack"] = (d(q_off, torch.int32), d(q_len, torch.int32), len(idx)) + extra
        args = (d(px, torch.float32), d(ids, torch.int32), d(pos, torch.int32), None, d(labels, torch.int32).reshape(-1), B, T)
    else:
        posd = torch.arange(T, dtype=torch.int32, device=dev)[None].expand(B, T).contiguous()
        args = (d(px, torch.float32), d(dec_in, torch.int32).reshape(-1), posd.reshape(-1), d(mask, torch.int32),
                d(labels, torch.int32).reshape(-1), B, T)
    return args, kw


def grad_distances(got, ref_g):
    """{leaf: max |got - ref| / max |ref|} over the leaves whose reference gradient is not analytically zero, and the cosine"""
    worst = {}
    for k, rg in ref_g.items():
        rg = torch.as_tensor(rg)
        gg = torch.from_numpy(np.asarray(got[k])).reshape(rg.shape)
        s = rg.abs().max().item()
        if s < 1e-6:
            continue
        worst[k] = ((gg - rg).abs().max() / s).item()
    a = torch.cat([torch.from_numpy(np.asarray(got[k])).reshape(-1).float() for k in ref_g])
    b = torch.cat([torch.as_tensor(v).reshape(-1).float() for v in ref_g.values()])
    return worst, torch.nn.functional.cosine_similarity(a, b, dim=0).item()


# ------------------------------------------------------------------------------------------------------------ fp32, decisive
@pytest.mark.parametrize("train,ls,compact", [(False, 0.0, False), (True, 0.0, False), (True, 0.1, False), (True, 0.1, True), (False, 0.0, True)])
def test_fp32_loss_and_grads_match_the_oracle_on_repeated_pixels(dev, train, ls, compact):
    """the bounds of test_loss_and_grads_match_oracle: loss 2e-5, every gradient leaf 5e-4 of its scale"""
    from oracle import train_ref

    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6)
    n_img, G, T = 2, 3, 12
    B = n_img * G
    px, labels, mask, dec_in = grouped(rc, n_img, G, T, seed=11)
    assert len({int(x) for x in mask.sum(1)}) > 2  # ragged
    seed = 4242 if train else None
    masks = oracle_masks(model, rc, seed, B, T) if train else None
    ref_loss, ref_g = train_ref.loss_and_grads(rc, p, px.repeat_interleave(G, 0), labels, mask, dec_in, masks, ls)
    args, kw = engine_args(model, px, labels, mask, dec_in, compact=compact, pack=False, G=G)
    loss = model.engine.loss_and_grads(*args, label_smoothing=ls, seed=seed, images=n_img, **kw)
    torch.cuda.synchronize()
    print(f"[captions_per_image fp32 train={train} ls={ls} compact={compact}] loss {loss.item():.7f} oracle {ref_loss.item():.7f}")
    assert abs(loss.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item())), (loss.item(), ref_loss.item())
    got = model.store.export_flat("grad")
    worst, _ = grad_distances(got, ref_g)
    for k, rg in ref_g.items():
        if rg.abs().max().item() < 1e-6:  # analytically zero (test_loss_and_grads_match_oracle): only fp noise on both sides
            assert np.abs(got[k]).max() < 1e-6, k
    print("  worst gradient leaves:", sorted(worst.items(), key=lambda kv: -kv[1])[:3])
    bad = {k: v for k, v in worst.items() if v > 5e-4}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]
    # loss_only: the evaluation pass (no dropout) on the same batch
    ref_eval = train_ref.loss_and_grads(rc, p, px.repeat_interleave(G, 0), labels, mask, dec_in, None, ls)[0]
    ev = model.engine.loss_only(*args, label_smoothing=ls, images=n_img, **kw)
    assert abs(ev.item() - ref_eval.item()) < 2e-5 * max(1.0, abs(ref_eval.item())), (ev.item(), ref_eval.item())


# ------------------------------------------------------------------------------------------------------------ bf16
def _bf16_case(dev, n_img, G, T, pack, seed, **over):
    """grouped and repeated-pixels passes of two identical bf16 models; (loss, grads) of both, the oracle's, and the eval losses"""
    from oracle import train_ref

    px, labels, mask, dec_in = None, None, None, None
    res = {}
    for form in ("grouped", "repeated"):
        rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0, **over)
        if px is None:
            px, labels, mask, dec_in = grouped(rc, n_img, G, T, seed=seed)
        g = G if form == "grouped" else 1
        pxf = px if form == "grouped" else px.repeat_interleave(G, 0)
        args, kw = engine_args(model, pxf, labels, mask, dec_in, compact=pack, pack=pack, G=g)
        im = dict(images=n_img) if form == "grouped" else {}
        loss = model.engine.loss_and_grads(*args, **im, **kw)
        torch.cuda.synchronize()
        grads = model.store.export_flat("grad")
        ev = model.engine.loss_only(*args, **im, **kw)
        res[form] = (loss.item(), grads, ev.item())
    ref_loss, ref_g = train_ref.loss_and_grads(rc, p, px.repeat_interleave(G, 0), labels, mask, dec_in)
    return res, ref_loss.item(), ref_g


def _check_bf16(tag, res, ref_loss, ref_g):
    """the bf16 bounds of test_loss_and_grads_match_oracle: loss 2e-2, every leaf 8e-2 of its scale, cosine > 0.995"""
    (lg, gg, eg), (lr, gr, er) = res["grouped"], res["repeated"]
    w_o, c_o = grad_distances(gg, ref_g)
    w_r, c_r = grad_distances(gg, {k: gr[k] for k in ref_g})
    print(f"[captions_per_image bf16 {tag}] loss grouped {lg:.5f} repeated {lr:.5f} oracle {ref_loss:.5f}; eval {eg:.5f} / {er:.5f}; "
          f"worst leaf vs oracle {max(w_o.values()):.4f} (cos {c_o:.5f}), vs the repeated step {max(w_r.values()):.4f} (cos {c_r:.5f})")
    assert abs(lg - ref_loss) < 2e-2 * max(1.0, abs(ref_loss)) and abs(lg - lr) < 2e-2 * max(1.0, abs(lr)), (lg, lr, ref_loss)
    assert abs(eg - er) < 2e-2 * max(1.0, abs(er)), (eg, er)
    for w, c in ((w_o, c_o), (w_r, c_r)):
        bad = {k: v for k, v in w.items() if v > 8e-2}
        assert not bad and c > 0.995, (sorted(bad.items(), key=lambda kv: -kv[1])[:8], c)


@pytest.mark.parametrize("pack", [True, False])
def test_bf16_grouped_step_matches_the_oracle_and_the_repeated_step(dev, pack):
    res, ref_loss, ref_g = _bf16_case(dev, 2, 3, 12, pack, seed=21)
    _check_bf16(f"pack={pack}", res, ref_loss, ref_g)


def test_bf16_beyond_one_tile_and_the_tiled_switch(dev, monkeypatch):
    """T = 72 > 64: an image's G captions are one sequence of the tiled kernels (packed rows regrouped); the same form at T = 12 under
    MIC_ATTN_SHARED=tiled"""
    res, ref_loss, ref_g = _bf16_case(dev, 2, 2, 72, True, seed=31, max_position_embeddings=80)
    _check_bf16("T=72 packed", res, ref_loss, ref_g)
    monkeypatch.setenv("MIC_ATTN_SHARED", "tiled")
    for pack in (True, False):
        res, ref_loss, ref_g = _bf16_case(dev, 2, 2, 12, pack, seed=32)
        _check_bf16(f"T=12 MIC_ATTN_SHARED=tiled pack={pack}", res, ref_loss, ref_g)


# ------------------------------------------------------------------------------------------------------------ Trainer
def _lr():
    from mic_amd import create_learning_rate_fn

    return create_learning_rate_fn(64, 2, 4, 0, 1e-3)


def test_trainer_steps_match_the_repeated_pixels_twin(dev):
    """three train steps and one eval step, bf16, same seed, dropout 0.1: the criteria of
    test_trainer_packs_rows_by_default_and_matches_the_padded_trainer (losses rtol 2e-3, eval loss 2e-3)"""
    from mic_amd import Trainer

    n_img, G, T = 2, 3, 12
    res = {}
    for form in ("grouped", "repeated"):
        rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        tr = Trainer(model, _lr(), seed=7)
        losses = []
        for s in range(3):
            px, labels, mask, dec_in = grouped(rc, n_img, G, T, seed=70 + 2 * s)
            b = bdict(px, labels, mask, dec_in, G) if form == "grouped" else bdict(px.repeat_interleave(G, 0), labels, mask, dec_in)
            losses.append(float(tr.train_step(b)["loss"]))
            assert tr._pack is not None and (len(tr._pack[0]) == 5) == (form == "grouped")
        res[form] = (losses, float(tr.eval_step(b)["loss"]))
    print("[captions_per_image trainer bf16]", res)
    assert np.allclose(res["grouped"][0], res["repeated"][0], rtol=2e-3), res
    assert abs(res["grouped"][1] - res["repeated"][1]) < 2e-3 * abs(res["repeated"][1]), res


def test_trainer_fp32_steps_match_the_oracles_adamw(dev):
    """test_train_steps_match_oracle_adamw with G = 3: loss within 5e-5, every weight within 2e-5 after three steps"""
    from mic_amd import Trainer, create_learning_rate_fn
    from mic_amd.params import flatten_tree
    from oracle import train_ref

    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    n_img, G, T = 2, 3, 12
    lr_fn = create_learning_rate_fn(train_ds_size=40, train_batch_size=4, num_train_epochs=1, num_warmup_steps=2, learning_rate=1e-3)
    tr = Trainer(model, lr_fn, weight_decay=0.01, label_smoothing_factor=0.0, seed=42)
    params = {k: v.clone() for k, v in p.items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(v) for k, v in p.items()}
    for step in range(3):
        px, labels, mask, dec_in = grouped(rc, n_img, G, T, seed=100 + 2 * step)
        out = tr.train_step(bdict(px, labels, mask, dec_in, G))
        ref_loss, g = train_ref.loss_and_grads(rc, params, px.repeat_interleave(G, 0), labels, mask, dec_in)
        lr = train_ref.linear_warmup_decay(step, 1e-3, 2, 10)
        assert abs(float(out["learning_rate"]) - lr) < 1e-9
        assert abs(float(out["loss"]) - ref_loss.item()) < 5e-5 * max(1.0, ref_loss.item())
        for k in params:
            params[k], m[k], v[k] = train_ref.adamw_update(params[k], g[k], m[k], v[k], step, lr, wd=0.01)
    gf = flatten_tree(model.params)
    for k, rv in params.items():
        d = (torch.from_numpy(gf[k]) - rv).abs().max().item()
        assert d < 2e-5, (k, d)


@pytest.mark.parametrize("case", ["accumulate", "clip", "frozen"])
def test_combinations_match_their_repeated_pixels_twin(dev, case):
    """one optimizer step each: accumulate_steps = 2, max_grad_norm = 0.5, a frozen image tower — bf16, dropout 0.1, the same seed;
    step loss(es), the clipped step's grad_norm and the eval loss behind the step within rtol 2e-3 of the twin's"""
    from mic_amd import Trainer
    from mic_amd.params import flatten_tree
    from mic_amd.train import ENCODER

    kw = {"accumulate": dict(accumulate_steps=2), "clip": dict(max_grad_norm=0.5),
          "frozen": dict(param_groups=[dict(match=ENCODER, frozen=True)])}[case]
    n_img, G, T = 2, 3, 12
    res = {}
    for form in ("grouped", "repeated"):
        rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        before = {k: v.copy() for k, v in flatten_tree(model.params).items()}
        tr = Trainer(model, _lr(), seed=9, **kw)
        outs = []
        for s in range(2 if case == "accumulate" else 1):
            px, labels, mask, dec_in = grouped(rc, n_img, G, T, seed=90 + 2 * s)
            b = bdict(px, labels, mask, dec_in, G) if form == "grouped" else bdict(px.repeat_interleave(G, 0), labels, mask, dec_in)
            out = tr.train_step(b)
            outs.append(float(out["loss"]))
        assert tr.step == 1
        if case == "clip":
            outs.append(float(out["grad_norm"]))
        outs.append(float(tr.eval_step(b)["loss"]))
        after = flatten_tree(model.params)
        if case == "frozen":
            assert tr._encoder_frozen and tr.skip_frozen_backward
            tower = [k for k in before if "/encoder/" in k or "vision" in k or "patch" in k]
            moved = [k for k in before if not np.array_equal(before[k], after[k])]
            assert tower and moved and not set(tower) & set(moved), (len(tower), sorted(set(tower) & set(moved))[:5])
        res[form] = outs
    print(f"[captions_per_image {case}]", res)
    assert np.allclose(res["grouped"], res["repeated"], rtol=2e-3), res


# ------------------------------------------------------------------------------------------------------------ the work is shared
def test_image_side_gemms_run_at_the_number_of_images(dev, monkeypatch):
    """every GEMM launch that touches the image tower's, the bridge's or the cross k/v projections' weights or weight gradients
    (forward, dX, dW) sees at most n_img * S rows — an implementation that repeats the pixels inside would show n_img * G * S"""
    import re

    from mic_amd import Trainer, ops
    from mic_amd.train import ENCODER

    n_img, G, T = 4, 4, 12
    rc, p, model = make_pair(torch.bfloat16, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    tr = Trainer(model, _lr())
    st = model.store
    S = st.S
    rup = lambda x: (x + 127) // 128 * 128  # noqa: E731
    assert rup(n_img * S) < rup(n_img * G * S)  # (the weight-gradient GEMMs reduce over the row count padded to 128)
    ranges = []
    for name, seg in st.segs.items():
        if re.fullmatch(ENCODER, name) or name.startswith("vp.") or re.fullmatch(r"dec\d+\.ckv\.[wb]", name):
            for buf in {id(t): t for t in (st.lp, st.master, st.grad) if t is not None}.values():
                a = buf.data_ptr() + seg.offset * buf.element_size()
                ranges.append((a, a + seg.numel * buf.element_size()))
    ranges.sort()

    def image_side(*ptrs):
        return any(p is not None and any(a <= p < e for a, e in ranges) for p in ptrs)

    seen = []  # (image side?, rows)

    def note(A, B, C, M, K, kmajor, k_valid, rowsum_k):
        rows = (k_valid or rowsum_k or K) if kmajor else M
        seen.append((image_side(A, B, C), rows, bool(kmajor and not (k_valid or rowsum_k))))

    real_gemm, real_grouped = ops.gemm, ops.gemm_grouped

    def gemm(a, b, out, M, N, K, **kw):
        note(a.data_ptr(), b.data_ptr(), out.data_ptr(), M, K, kw.get("a_kmajor") and kw.get("b_kmajor"), kw.get("k_valid", 0), kw.get("rowsum_k", 0))
        return real_gemm(a, b, out, M, N, K, **kw)

    def gemm_grouped(arg_list):
        for g in arg_list:
            note(g.A, g.B, g.C, g.M, g.K, g.a_kmajor and g.b_kmajor, g.k_valid, g.rowsum_k)
        return real_grouped(arg_list)

    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(ops, "gemm_grouped", gemm_grouped)
    px, labels, mask, dec_in = grouped(rc, n_img, G, T, seed=41)
    tr.train_step(bdict(px, labels, mask, dec_in, G))
    tr.eval_step(bdict(px, labels, mask, dec_in, G))
    torch.cuda.synchronize()
    img = [(rows, padded) for side, rows, padded in seen if side]
    dec = [rows for side, rows, _ in seen if not side]
    # forward (2 layers x 4 + patch + bridge + ckv) twice, dX and dW once: dozens of launches, and the decoder's are there to compare
    assert len(img) >= 30 and dec and max(dec) > n_img * S, (len(img), len(dec))
    over = [(rows, padded) for rows, padded in img if rows > (rup(n_img * S) if padded else n_img * S)]
    assert not over, over


# ------------------------------------------------------------------------------------------------------------ default untouched
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_default_path_gives_the_same_bits(dev, dtype):
    """a batch without the key and one with captions_per_image = 1 on the same Trainer state: the same loss bits and the same gradient
    bytes as the engine call the step has always made.  Bytes are compared where the step itself is reproducible from run to run: every
    segment the GEMMs write.  The segments summed with fp32 atomics in an order that changes between two runs of the SAME call (the
    embedding scatters into `shared` / `dec.pos`, `flb`, and the bias / LayerNorm region behind ParamStore.atomic_begin) are compared
    within 1e-5 of their scale, the size of such a reordering."""
    from mic_amd import Trainer

    runs = []
    for key in (None, 1, "engine"):
        rc, p, model = make_pair(dtype, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1)
        tr = Trainer(model, _lr(), seed=3)
        px, labels, mask, dec_in = batch(rc, 4, 12, seed=55)
        b = bdict(px, labels, mask, dec_in, key if key != "engine" else None)
        if key == "engine":  # today's call, spelled out: _prep, then loss_and_grads without `images`
            from mic_amd.train import virtual_rank_dropout_seed

            a = tr._prep(b)
            seed = virtual_rank_dropout_seed(tr.seed, tr.rank, tr.step, 1, 0)
            eng = model.engine
            if tr._pack is not None:
                pack, ids_p, pos_p = tr._pack
                assert len(pack) == 3
                loss = eng.loss_and_grads(a[0], ids_p, pos_p, None, a[1].reshape(-1), a[5], a[6], label_smoothing=tr.ls, seed=seed,
                                          rows=tr._rows, row_labels=tr._row_labels, pack=pack)
            else:
                loss = eng.loss_and_grads(a[0], a[3].reshape(-1), a[4].reshape(-1), a[2], a[1].reshape(-1), a[5], a[6],
                                          label_smoothing=tr.ls, seed=seed, rows=tr._rows, row_labels=tr._row_labels)
            loss = float(loss)
        else:
            loss = float(tr.train_step(b)["loss"])
            assert tr._images is None
        torch.cuda.synchronize()
        runs.append((np.float32(loss).tobytes(), model.store.grad.cpu().numpy()))
    assert runs[0][0] == runs[1][0] == runs[2][0], "loss bits differ"
    st = model.store
    exact = 0
    for name, seg in st.segs.items():
        sl = slice(seg.offset, seg.offset + seg.numel)
        ref = runs[2][1][sl]
        for other, what in ((runs[0][1][sl], "a batch without the key"), (runs[1][1][sl], "captions_per_image = 1")):
            if name in ("shared", "dec.pos", "flb") or seg.offset >= st.atomic_begin:
                assert np.abs(other - ref).max() <= 1e-5 * max(np.abs(ref).max(), 1e-12), (name, what)
            else:
                exact += 1
                assert other.tobytes() == ref.tobytes(), f"{name}: gradient bytes of {what} differ from the plain engine call"
    assert exact >= 2 * 20  # (the reduced model: 24 weight matrices)


# ------------------------------------------------------------------------------------------------------------ two ranks
def _rank_shards(rc, n_img, G, T):
    """two shards with the same number of valid tokens (rank 1's captions are rank 0's in another order, on other images): the mean
    over the ranks of their per-rank mean losses is then the mean over the concatenated batch"""
    px0, labels, mask, dec_in = grouped(rc, n_img, G, T, seed=600)
    px1 = batch(rc, n_img, T, seed=601)[0]
    perm = torch.roll(torch.arange(n_img * G), 1)
    return [(px0, labels, mask, dec_in), (px1, labels[perm], mask[perm], dec_in[perm])]


def _rank_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import mic_amd  # noqa: F401
        from mic_amd import Trainer, create_learning_rate_fn
        from mic_amd.params import flatten_tree

        dev = torch.device("cuda:0")
        rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
        tr = Trainer(model, create_learning_rate_fn(40, 4, 1, 0, 1e-3), weight_decay=0.01, seed=42, bucket_mb=0.25)
        px, labels, mask, dec_in = _rank_shards(rc, 2, 2, 12)[rank]
        out = tr.train_step(bdict(px, labels, mask, dec_in, 2))
        torch.cuda.synchronize()
        q.put((rank, float(out["loss"]), {k: v.copy() for k, v in flatten_tree(model.params).items()}))
    finally:
        dist.destroy_process_group()


def test_two_ranks_stay_identical_and_match_the_one_process_step(dev):
    """two gloo ranks on one device, G = 2 on both: identical replicas after the step, equal to the one-process step on the
    concatenated batch within the bound of tests/test_ddp_gpu.py (weights 1e-4, loss 5e-5)"""
    import torch.multiprocessing as mp

    from mic_amd import Trainer, create_learning_rate_fn
    from mic_amd.params import flatten_tree

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31100 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda r: r[0])
    for pr in procs:
        pr.join(timeout=60)
    (_, l0, w0), (_, l1, w1) = res
    assert l0 == l1 and all(np.array_equal(w0[k], w1[k]) for k in w0), "the replicas differ"
    rc, p, model = make_pair(torch.float32, dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.0)
    tr = Trainer(model, create_learning_rate_fn(40, 4, 1, 0, 1e-3), weight_decay=0.01, seed=42, bucket_mb=0.25)
    a, b = _rank_shards(rc, 2, 2, 12)
    cat = [torch.cat((x, y)) for x, y in zip(a, b)]
    out = tr.train_step(bdict(*cat, 2))
    one = flatten_tree(model.params)
    assert abs(float(out["loss"]) - l0) < 5e-5, (float(out["loss"]), l0)
    worst = max((float(np.abs(one[k] - w0[k]).max()), k) for k in one)
    print("[captions_per_image two ranks] worst weight distance to the one-process step:", worst)
    assert worst[0] < 1e-4, worst
