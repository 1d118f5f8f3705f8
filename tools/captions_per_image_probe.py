"""What batch["captions_per_image"] = G buys at the bench workload: the grouped step (n_img = rows / G images, G captions each) against
the repeated-pixels step (the same n_img images, each put into the batch G times) of the same tree.

Full-size model, bf16, 64 caption rows per step, seq 64, the bench's ragged captions, device-resident batches with the collate extras
(bench.py's train leg; the host's decode and upload of the repeated images are therefore NOT in these figures).  ONE process and ONE
Trainer: the two forms differ only in the batch they are handed.  After warm-up of every form, the forms are timed alternately with
device events, one event between any two `train_step` calls:

  G = 4 (16 images): repeated | grouped (one-tile shared-K/V kernels) | grouped with MIC_ATTN_SHARED=tiled, `--alternations` times
  G = 2 and G = 8:   repeated | grouped, likewise

Reported per form: ms per step (median over all timed steps), caption rows/s, and the spread = the largest distance between the
per-alternation medians of one form.  The grouped step counts as faster only if the gain exceeds that spread.

  python tools/captions_per_image_probe.py [--rows 64] [--alternations 3] [--steps 6] [--small] [--json out.json]
  rocprofv3 --kernel-trace --stats -- python tools/captions_per_image_probe.py --trace grouped|repeated|tiled   (G = 4, a few steps:
      the kernels' own times, summarised by tools/rocpd_stats.py)
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
    ap.add_argument("--rows", type=int, default=64, help="caption rows per step")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6, help="timed steps per window")
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--trace", default=None, choices=["grouped", "repeated", "tiled"], help="G = 4, warm-up + 4 steps of one form, nothing timed")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.alternations >= 3 and args.rows % 8 == 0

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
    R, T = args.rows, 64
    lr_fn = create_learning_rate_fn(train_ds_size=10_000_000, train_batch_size=R, num_train_epochs=7, num_warmup_steps=1000, learning_rate=5e-5)
    tr = Trainer(model, lr_fn, seed=42)
    eng = model.engine
    V, img = cfg.mbart_config.vocab_size, cfg.clip_vision_config.image_size

    def forms(G):
        """two batches per form: {"repeated": [...], "grouped": [...]} on the same captions and the same n_img images"""
        out = {"repeated": [], "grouped": []}
        for i in range(2):
            b = bench.synth_batch(R, T, V, img, 1234 + i)
            base = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k != "pixel_values"}
            idx, rl = loss_rows(b["attention_mask"], b["input_ids"])
            base["loss_rows"] = (torch.from_numpy(idx).to(dev), torch.from_numpy(rl).to(dev))
            pk = packed_rows(b["attention_mask"], b["decoder_input_ids"])
            if pk is not None:
                # the description stays on the host for the grouped form (its regrouping per image is host arithmetic)
                base["packed_rows"] = tuple(torch.from_numpy(t).to(dev) for t in pk)
            px = torch.from_numpy(b["pixel_values"][: R // G]).to(dev)
            out["repeated"].append(dict(base, pixel_values=px.repeat_interleave(G, 0).contiguous()))
            g = dict(base, pixel_values=px, captions_per_image=G)
            if pk is not None:
                g["packed_rows"] = pk
            out["grouped"].append(g)
        return out

    def window(batches, n_calls, tiled=False):
        eng.attn_shared_tiled = tiled
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_calls + 1)]
        ev[0].record()
        for i in range(n_calls):
            tr.train_step(batches[i % 2])
            ev[i + 1].record()
        torch.cuda.synchronize()
        eng.attn_shared_tiled = False
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n_calls)]

    if args.trace:
        f = forms(4)
        window(f["repeated" if args.trace == "repeated" else "grouped"], 3 + 4, tiled=args.trace == "tiled")
        return

    res = {"probe": "captions_per_image", "rows": R, "seq": T, "alternations": args.alternations, "steps_per_window": args.steps,
           "small_debug_model": bool(args.small), "cases": {}}
    for G in (4, 2, 8):
        f = forms(G)
        legs = [("repeated", f["repeated"], False), ("grouped", f["grouped"], False)] + ([("grouped_tiled", f["grouped"], True)] if G == 4 else [])
        for _ in range(2):  # warm-up of every form (buffers keyed on the row counts, GEMM plans)
            for _, bt, tiled in legs:
                window(bt, 3, tiled)
        meds = {name: [] for name, _, _ in legs}
        allms = {name: [] for name, _, _ in legs}
        for _ in range(args.alternations):
            for name, bt, tiled in legs:
                w = window(bt, args.steps, tiled)
                meds[name].append(statistics.median(w))
                allms[name] += w
        case = {"images": R // G}
        for name in meds:
            ms = statistics.median(allms[name])
            case[name] = {"ms_per_step": round(ms, 3), "caption_rows_per_s": round(R / ms * 1e3, 1),
                          "per_alternation_ms": [round(x, 3) for x in meds[name]], "spread_ms": round(max(meds[name]) - min(meds[name]), 3)}
        spread = max(case[n]["spread_ms"] for n in meds)
        gain = case["repeated"]["ms_per_step"] - case["grouped"]["ms_per_step"]
        case.update(gain_ms=round(gain, 3), spread_ms=round(spread, 3), faster_by_more_than_the_spread=bool(gain > spread))
        res["cases"][f"G={G}"] = case
        line = ", ".join(f"{n} {case[n]['ms_per_step']:.3f} ms ({case[n]['caption_rows_per_s']:.0f} rows/s)" for n in meds)
        print(f"G = {G} ({R // G} images): {line}; grouped - repeated = {-gain:+.3f} ms against a spread of {spread:.3f} ms -> "
              + ("faster by more than the spread" if gain > spread else "NOT faster by more than the spread"))
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
