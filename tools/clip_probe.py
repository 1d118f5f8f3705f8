"""What global-norm gradient clipping (`Trainer(max_grad_norm=c)`) costs at the bench workload: a plain `Trainer.train_step` against a
clipped one.

Full-size model, bf16, batch 64, seq 64, ragged captions, device-resident batches with the collate extras (bench.py's train leg).
ONE process and ONE Trainer (a second Trainer in a process shifts how its streams map onto hardware queues, `ops.role_stream`): it
is built with `max_grad_norm=c` and switched to the plain step for the plain windows by restoring the state the constructor derives
from the option (`mode()` below) — `train_step` then takes the path of a Trainer built without the keyword, launch for launch.
After warm-up of both forms the two are timed alternately with device events, one event between any two calls (`train_step` joins
its side streams into the caller's stream before it returns, so the events see the optimizer too).  Then, in the same process, the
stand-alone times of the launches clipping adds or exposes: one whole-buffer `adamw`, one whole-buffer `grad_sumsq`, one `clip_coef`.

With clipping AdamW cannot start before the last gradient exists: it no longer hides beside backward, and one whole-buffer pass is
exposed behind it; the per-bucket sums of squares (4 B/element) should hide as `acc += g` does.  Expected: the step grows by no more
than the stand-alone AdamW time plus the `clip_coef` launch, with 10 % of that sum allowed on top.  The verdict line says which side
of it the run fell on.

  python tools/clip_probe.py [--max-grad-norm 1.0] [--batch 64] [--steps 8] [--alternations 3] [--small] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8, help="train steps per window")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.steps > 1 and args.alternations >= 3

    import torch

    import bench
    from mic_amd import (CLIPVisionMBartConfig, FlaxCLIPVisionMBartForConditionalGeneration, Trainer, create_learning_rate_fn, loss_rows, ops,
                         packed_rows)

    dev = torch.device("cuda:0")
    if args.small:
        cfg = CLIPVisionMBartConfig(mbart_config=dict(vocab_size=5003, d_model=256, decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=512),
                                    clip_vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                            image_size=64, patch_size=32))
    else:
        cfg = CLIPVisionMBartConfig(mbart_config={}, clip_vision_config={})
    model = FlaxCLIPVisionMBartForConditionalGeneration(cfg, seed=0, dtype=torch.bfloat16, device=dev)
    K, B, T = args.steps, args.batch, 64
    lr_fn = create_learning_rate_fn(train_ds_size=10_000_000, train_batch_size=B, num_train_epochs=7, num_warmup_steps=1000, learning_rate=5e-5)
    tr = Trainer(model, lr_fn, seed=42, max_grad_norm=args.max_grad_norm)
    r, st = tr.reducer, model.store
    assert tr.overlap_optimizer and r.on_ready is not None and not tr._split_shared
    V, img = cfg.mbart_config.vocab_size, cfg.clip_vision_config.image_size
    batches = []
    for i in range(2):
        b = bench.synth_batch(B, T, V, img, 1234 + i)
        db = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
        idx, rl = loss_rows(b["attention_mask"], b["input_ids"])
        db["loss_rows"] = (torch.from_numpy(idx).to(dev), torch.from_numpy(rl).to(dev))
        pk = packed_rows(b["attention_mask"], b["decoder_input_ids"])
        if pk is not None:
            db["packed_rows"] = tuple(torch.from_numpy(t).to(dev) for t in pk)
        batches.append(db)

    # the two forms of everything Trainer.__init__ derives from max_grad_norm
    sb, se, width = tr._sh
    assert (se - sb) % width == 0
    clip_state = dict(_split_shared=False, _row_flag=None, _clip_out=tr._clip_out)
    clip_red = dict(on_ready=r.on_ready, ready_when=list(r.ready_when))
    plain_state = dict(_split_shared=True, _row_flag=torch.zeros((se - sb) // width, dtype=torch.uint8, device=dev), _clip_out=None)
    plain_red = dict(on_ready=lambda b, e: tr._adamw_slice(b, e),
                     ready_when=["next" if (b < se and e > sb) else "exchanged" for (b, e) in tr.buckets])

    def mode(clip):
        """clip=False: the plain step of a Trainer without max_grad_norm (per-bucket AdamW, the tied embedding's rows split)"""
        for k, v in (clip_state if clip else plain_state).items():
            setattr(tr, k, v)
        for k, v in (clip_red if clip else plain_red).items():
            setattr(r, k, v)

    def window(n_calls):
        """n_calls train_step calls, an event between any two: ms of each call on the device"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_calls + 1)]
        ev[0].record()
        outs = []
        for i in range(n_calls):
            outs.append(tr.train_step(batches[i % 2]))
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n_calls)], outs

    for clip in (False, True, False, True):  # warm-up of both forms (buffers, plans, the k-major embedding copy)
        mode(clip)
        window(K)
    plain, clipped, norms = [], [], []
    for _ in range(args.alternations):
        mode(False)
        ms, outs = window(K)
        assert all("grad_norm" not in o for o in outs)
        plain.append(ms)
        mode(True)
        ms, outs = window(K)
        norms += [float(o["grad_norm"]) for o in outs]
        clipped.append(ms)

    def alone(fn, reps=7):
        """median ms of one launch on an otherwise idle device"""
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return statistics.median(out)

    lp = None if st.lp is st.master else st.lp
    parts = torch.empty(ops.grad_sumsq_slots(st.numel), dtype=torch.float32, device=dev)
    out2 = torch.empty(2, dtype=torch.float32, device=dev)
    ms_adamw = alone(lambda: ops.adamw(st.master, st.m, st.v, st.grad, lp, tr.hyper, tr.b1, tr.b2, tr.eps, tr.wd, grad_scale=tr._gscale))
    ms_adamw_clip = alone(lambda: ops.adamw_clip(st.master, st.m, st.v, st.grad, lp, tr.hyper, tr._clip_out[1:2], tr.b1, tr.b2, tr.eps, tr.wd))
    ms_sumsq = alone(lambda: ops.grad_sumsq(st.grad, parts))
    ms_coef = alone(lambda: ops.clip_coef(tr._clip_partials, tr._clip_slots, tr._gscale, args.max_grad_norm, out2))

    a_tot, b_tot = [sum(w) for w in plain], [sum(w) for w in clipped]
    a_med = statistics.median([x for w in plain for x in w])
    b_med = statistics.median([x for w in clipped for x in w])
    spread = max(max(a_tot) - min(a_tot), max(b_tot) - min(b_tot)) / K
    allowed = 1.10 * (ms_adamw + ms_coef)
    r3 = lambda xs: [round(x, 3) for x in xs]
    res = {"probe": "clip", "max_grad_norm": args.max_grad_norm, "batch": B, "seq": T, "steps_per_window": K, "alternations": args.alternations,
           "small_debug_model": bool(args.small), "buckets": len(tr.buckets), "partial_slots": int(tr._clip_slots), "elements": int(st.numel),
           "ms_per_plain_step": round(a_med, 3), "ms_per_clipped_step": round(b_med, 3), "clipped_minus_plain_ms": round(b_med - a_med, 3),
           "ms_plain_windows": r3(a_tot), "ms_clipped_windows": r3(b_tot), "spread_ms_per_step": round(spread, 3),
           "ms_adamw_whole_buffer_alone": round(ms_adamw, 3), "ms_adamw_clip_whole_buffer_alone": round(ms_adamw_clip, 3),
           "ms_grad_sumsq_whole_buffer_alone": round(ms_sumsq, 3), "ms_clip_coef_alone": round(ms_coef, 4),
           "allowed_growth_ms": round(allowed, 3), "within_expectation": bool(b_med - a_med <= allowed),
           "images_per_s_plain": round(B / a_med * 1e3, 1), "images_per_s_clipped": round(B / b_med * 1e3, 1),
           "grad_norm_first_last": [norms[0], norms[-1]]}
    print(f"plain step {a_med:.3f} ms, clipped step {b_med:.3f} ms: +{b_med - a_med:.3f} ms; alone: adamw {ms_adamw:.3f} ms (adamw_clip "
          f"{ms_adamw_clip:.3f}), grad_sumsq {ms_sumsq:.3f} ms, clip_coef {ms_coef:.4f} ms over {tr._clip_slots} slots")
    print(f"expected growth <= 1.10 x (adamw + clip_coef) = {allowed:.3f} ms -> " + ("within it" if res["within_expectation"] else "LARGER than expected"))
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
