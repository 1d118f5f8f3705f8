"""What batch["loss_weights"] costs at the bench workload, and what one self-critical iteration is made of.

Full-size model, bf16, 64 caption rows per step, seq 64, the bench's ragged captions, device-resident batches with the collate extras
(bench.py's train leg).  ONE process and ONE Trainer: the two forms differ only in the batch they are handed — `weighted` carries
batch["loss_weights"], a device tensor of one fp32 weight per caption row (both signs, a zero among them), `plain` does not.  After
warm-up of both forms they are timed alternately with device events, one event between any two `train_step` calls, `--alternations`
times.  Reported per form: ms per step (median over all timed steps) and the spread = the largest distance between the
per-alternation medians of one form.  The weights count as free only if the difference stays inside that spread; the code predicts
level (one fp32 load per 64 x 512 tile row in the CE backward, two small torch launches in `_prep`).

  --scst: one `self_critical_batch` + `train_step` iteration at 16 images x 4 samples, after one warm-up iteration: wall time of the
  sampling (generate + the host copy of the sequences), of the host reward (the number of ids >= V / 2: a stand-in for the caller's
  metric) and of the step, each closed by a device synchronisation.  Informational, no bound.

  python tools/loss_weights_probe.py [--rows 64] [--alternations 3] [--steps 6] [--scst] [--small] [--json out.json]

(The plain step against the parent commit is measured with bench.py in alternated processes, not here: profiles/NOTES_r21.md.)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64, help="caption rows per step")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per window")
    ap.add_argument("--scst", action="store_true", help="also time one self-critical iteration (16 images x 4 samples)")
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.alternations >= 3 and args.rows % 8 == 0

    import numpy as np
    import torch

    import bench
    from mic_amd import (CLIPVisionMBartConfig, FlaxCLIPVisionMBartForConditionalGeneration, Trainer, create_learning_rate_fn, loss_rows,
                         packed_rows)
    from mic_amd.evaluation import scst_advantages, self_critical_batch, sequences_to_score_inputs

    dev = torch.device("cuda:0")
    if args.small:
        cfg = CLIPVisionMBartConfig(mbart_config=dict(vocab_size=5003, d_model=256, decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=512),
                                    clip_vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                            image_size=64, patch_size=32))
    else:
        cfg = CLIPVisionMBartConfig(mbart_config={}, clip_vision_config={})
    model = FlaxCLIPVisionMBartForConditionalGeneration(cfg, seed=0, dtype=torch.bfloat16, device=dev)
    R, T = args.rows, 64
    lr_fn = create_learning_rate_fn(train_ds_size=10_000_000, train_batch_size=R, num_train_epochs=7, num_warmup_steps=1000, learning_rate=5e-5)
    tr = Trainer(model, lr_fn, seed=42)
    V, img = cfg.mbart_config.vocab_size, cfg.clip_vision_config.image_size

    forms = {"plain": [], "weighted": []}
    for i in range(2):
        b = bench.synth_batch(R, T, V, img, 1234 + i)
        base = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
        idx, rl = loss_rows(b["attention_mask"], b["input_ids"])
        base["loss_rows"] = (torch.from_numpy(idx).to(dev), torch.from_numpy(rl).to(dev))
        pk = packed_rows(b["attention_mask"], b["decoder_input_ids"])
        if pk is not None:
            base["packed_rows"] = tuple(torch.from_numpy(t).to(dev) for t in pk)
        w = np.random.default_rng(i).standard_normal(R).astype(np.float32)
        w[0] = 0.0
        forms["plain"].append(base)
        forms["weighted"].append(dict(base, loss_weights=torch.from_numpy(w).to(dev)))

    def window(batches, n_calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_calls + 1)]
        ev[0].record()
        for i in range(n_calls):
            tr.train_step(batches[i % 2])
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n_calls)]

    res = {"probe": "loss_weights", "rows": R, "seq": T, "alternations": args.alternations, "steps_per_window": args.steps,
           "small_debug_model": bool(args.small)}
    for _ in range(2):  # warm-up of both forms
        for name in forms:
            window(forms[name], 3)
    meds = {name: [] for name in forms}
    allms = {name: [] for name in forms}
    for _ in range(args.alternations):
        for name in forms:
            w = window(forms[name], args.steps)
            meds[name].append(statistics.median(w))
            allms[name] += w
    for name in forms:
        ms = statistics.median(allms[name])
        res[name] = {"ms_per_step": round(ms, 3), "caption_rows_per_s": round(R / ms * 1e3, 1),
                     "per_alternation_ms": [round(x, 3) for x in meds[name]], "spread_ms": round(max(meds[name]) - min(meds[name]), 3)}
    spread = max(res[n]["spread_ms"] for n in forms)
    cost = res["weighted"]["ms_per_step"] - res["plain"]["ms_per_step"]
    res.update(cost_ms=round(cost, 3), spread_ms=round(spread, 3), level_within_the_spread=bool(abs(cost) <= spread))
    print(f"plain {res['plain']['ms_per_step']:.3f} ms, weighted {res['weighted']['ms_per_step']:.3f} ms: weighted - plain = {cost:+.3f} ms "
          f"against a spread of {spread:.3f} ms -> " + ("level" if abs(cost) <= spread else "NOT level"))

    if args.scst:
        n_img, n = 16, 4
        px = torch.from_numpy(bench.synth_batch(n_img, T, V, img, 99)["pixel_values"]).to(dev)
        half = V // 2
        split = {}

        def sync():
            torch.cuda.synchronize()
            return time.perf_counter()

        for it in range(2):  # the first iteration warms the decode plan and the buffers of this batch shape
            t0 = sync()
            gen = model.generate(px, do_sample=True, num_beams=1, num_return_sequences=n, prng_key=7 + it, max_length=T)
            seq = np.asarray(gen.sequences.cpu())
            t1 = sync()
            rewards = (seq >= half).sum(1).astype(np.float32)
            mc = cfg.mbart_config
            dec_in, labels, mask = sequences_to_score_inputs(seq, mc.eos_token_id, mc.pad_token_id)
            b = {"pixel_values": px, "input_ids": labels, "attention_mask": mask, "decoder_input_ids": dec_in, "captions_per_image": n,
                 "loss_weights": scst_advantages(rewards, n)}
            t2 = sync()
            out = tr.train_step(b)
            t3 = sync()
            split = {"sampling_ms": round((t1 - t0) * 1e3, 2), "host_reward_and_batch_ms": round((t2 - t1) * 1e3, 2),
                     "train_step_ms": round((t3 - t2) * 1e3, 2), "total_ms": round((t3 - t0) * 1e3, 2), "loss": float(out["loss"]),
                     "valid_tokens": int(mask.sum())}
        # the helper itself, end to end (the same three stages behind one call)
        t0 = sync()
        b, _ = self_critical_batch(model, px, lambda s: (s >= half).sum(1), n, prng_key=11, max_length=T)
        tr.train_step(b)
        split["self_critical_batch_plus_step_ms"] = round((sync() - t0) * 1e3, 2)
        res["scst_16x4"] = split
        print("self-critical iteration, 16 images x 4 samples:", split)
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
