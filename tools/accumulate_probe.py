"""What gradient accumulation costs at the bench workload: a plain `Trainer.train_step` against one accumulation of N micro-steps.

Full-size model, bf16, batch 64, seq 64, ragged captions, device-resident batches with the collate extras (bench.py's train leg).
ONE process and ONE Trainer (a second Trainer in a process shifts how its streams map onto hardware queues, `ops.role_stream`): it
is built with `accumulate_steps=N` and switched to 1 for the plain windows — `train_step` then takes the path of a Trainer built
without the keyword, launch for launch (only the value of grad_scale is restored by hand).  After warm-up of both forms the two are
timed alternately with device events, one event between any two calls (`train_step` joins its side streams into the caller's stream
before it returns, so the events see the optimizer passes too):

  A: N plain steps          -> ms per plain step
  B: one accumulation of N  -> ms per non-final micro-step, ms of the final micro-step, images/s at global batch N * batch

From byte counts a non-final micro-step moves 12 B/element on the optimizer stream where a plain step moves 30, and the final one
4 B/element more than a plain step, all beside backward: B should cost no more than A.  The margin allowed over that is three times
the spread the probe observes between its own alternations; the verdict line says which side of it the run fell on.

  python tools/accumulate_probe.py [--n 8] [--batch 64] [--alternations 3] [--small] [--json out.json]
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
    ap.add_argument("--n", type=int, default=8, help="micro-steps per optimizer step")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.n > 1 and args.alternations >= 3

    import torch

    import bench
    from mic_amd import (CLIPVisionMBartConfig, FlaxCLIPVisionMBartForConditionalGeneration, Trainer, create_learning_rate_fn, loss_rows,
                         packed_rows)

    dev = torch.device("cuda:0")
    if args.small:
        cfg = CLIPVisionMBartConfig(mbart_config=dict(vocab_size=5003, d_model=256, decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=512),
                                    clip_vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                            image_size=64, patch_size=32))
    else:
        cfg = CLIPVisionMBartConfig(mbart_config={}, clip_vision_config={})
    model = FlaxCLIPVisionMBartForConditionalGeneration(cfg, seed=0, dtype=torch.bfloat16, device=dev)
    N, B, T = args.n, args.batch, 64
    lr_fn = create_learning_rate_fn(train_ds_size=10_000_000, train_batch_size=B * N, num_train_epochs=7, num_warmup_steps=1000, learning_rate=5e-5)
    tr = Trainer(model, lr_fn, seed=42, accumulate_steps=N)
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

    def mode(n):
        """n = 1: the plain step of a Trainer without accumulation; n = N: micro-steps"""
        assert tr._micro == 0
        tr.accumulate_steps, tr._gscale = n, 1.0 / (tr.world * n)

    def window(n_calls):
        """n_calls train_step calls, an event between any two: ms of each call on the device"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_calls + 1)]
        ev[0].record()
        for i in range(n_calls):
            tr.train_step(batches[i % 2])
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n_calls)]

    for n in (1, N, 1, N):  # warm-up of both forms (buffers, plans, the k-major embedding copy)
        mode(n)
        window(N)
    plain, micro = [], []
    for _ in range(args.alternations):
        mode(1)
        plain.append(window(N))
        mode(N)
        micro.append(window(N))
        assert tr._micro == 0
    a_tot, b_tot = [sum(w) for w in plain], [sum(w) for w in micro]
    spread = max(max(a_tot) - min(a_tot), max(b_tot) - min(b_tot))
    a_med, b_med = statistics.median(a_tot), statistics.median(b_tot)
    r3 = lambda xs: [round(x, 3) for x in xs]
    res = {"probe": "accumulate", "n": N, "batch": B, "seq": T, "alternations": args.alternations, "small_debug_model": bool(args.small),
           "ms_per_plain_step": round(statistics.median([x for w in plain for x in w]), 3),
           "ms_per_non_final_micro_step": round(statistics.median([x for w in micro for x in w[:-1]]), 3),
           "ms_final_micro_step": round(statistics.median([w[-1] for w in micro]), 3),
           "ms_n_plain_steps": r3(a_tot), "ms_one_accumulation": r3(b_tot), "spread_ms": round(spread, 3),
           "images_per_s_plain": round(N * B / a_med * 1e3, 1), "images_per_s_at_global_batch": round(N * B / b_med * 1e3, 1),
           "global_batch": N * B, "accumulation_minus_plain_ms": round(b_med - a_med, 3), "margin_ms": round(3 * spread, 3),
           "within_margin": bool(b_med <= a_med + 3 * spread)}
    print(f"plain step {res['ms_per_plain_step']:.3f} ms; non-final micro-step {res['ms_per_non_final_micro_step']:.3f} ms; final micro-step "
          f"{res['ms_final_micro_step']:.3f} ms; {res['images_per_s_at_global_batch']:.1f} images/s at global batch {N * B} "
          f"({res['images_per_s_plain']:.1f} plain at batch {B})")
    print(f"{N} plain steps {r3(a_tot)} ms, one accumulation of {N} {r3(b_tot)} ms: accumulation - plain = {res['accumulation_minus_plain_ms']:+.3f} ms "
          f"against a margin of 3 x {spread:.3f} ms -> " + ("within the margin" if res["within_margin"] else "SLOWER than the margin allows"))
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
