"""What model.score costs at the bench workload, and what its two head forms cost against each other and against the evaluation pass
whose forward they share.

Full-size model, bf16, 64 caption rows, seq 64, the bench's ragged captions; pixels device-resident, labels / masks on the host as a
caller holds them (score's collate arithmetic — loss_rows, packed_rows, a few small uploads — is inside its figure; eval_step gets the
collate extras precomputed, as in bench.py's legs).  ONE process, after warm-up of every form the forms are timed alternately with
device events, one event between any two calls:

  score (logits-free head) | score with MIC_SCORE_HEAD=materialised | Trainer.eval_step on the same batch        `--alternations` times
  score of 16 images x 16 candidates (candidates_per_image=16) | score of the same 256 rows on 256 repeated images, likewise

Reported per form: ms per call (median over all timed calls) and the spread = the largest distance between the per-alternation medians
of one form.  A form counts as faster only if the gain exceeds the spread.

  python tools/score_probe.py [--rows 64] [--alternations 3] [--calls 6] [--small] [--json out.json]
  rocprofv3 --kernel-trace --stats -- python tools/score_probe.py --trace      (warm-up + 4 calls of each head form, nothing timed:
      gemm_d2_kernel<2> against <1>, summarised by tools/rocpd_stats.py)
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
    ap.add_argument("--rows", type=int, default=64, help="caption rows per call")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--calls", type=int, default=6, help="timed calls per window")
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--trace", action="store_true", help="warm-up + 4 calls of each head form, nothing timed")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.alternations >= 3

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
    tr = Trainer(model, create_learning_rate_fn(10_000_000, R, 7, 1000, 5e-5), seed=42)
    V, img = cfg.mbart_config.vocab_size, cfg.clip_vision_config.image_size

    def batches(rows, n_img):
        """two (score arguments, eval batch) pairs on `rows` captions and `n_img` images"""
        out = []
        for i in range(2):
            b = bench.synth_batch(rows, T, V, img, 1234 + i)
            px = torch.from_numpy(b["pixel_values"][:n_img]).to(dev)
            ev = {k: torch.from_numpy(v).to(dev) for k, v in b.items() if k != "pixel_values"}
            idx, rl = loss_rows(b["attention_mask"], b["input_ids"])
            ev["loss_rows"] = (torch.from_numpy(idx).to(dev), torch.from_numpy(rl).to(dev))
            pk = packed_rows(b["attention_mask"], b["decoder_input_ids"])
            if pk is not None:
                ev["packed_rows"] = tuple(torch.from_numpy(t).to(dev) for t in pk)
            ev["pixel_values"] = px
            out.append((px, b["input_ids"], b["attention_mask"], b["decoder_input_ids"], ev))
        return out

    def window(fn, bt, n_calls):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_calls + 1)]
        ev[0].record()
        for i in range(n_calls):
            fn(bt[i % 2])
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n_calls)]

    repeated_px = {}  # (built once per batch, outside the timed calls)

    def scorer(head, G=1, repeat=1):
        def fn(b):
            px, labels, mask, dec_in, _ = b
            if repeat > 1:
                if id(px) not in repeated_px:
                    repeated_px[id(px)] = px.repeat_interleave(repeat, 0).contiguous()
                px = repeated_px[id(px)]
            if head == "materialised":
                os.environ["MIC_SCORE_HEAD"] = "materialised"
            else:
                os.environ.pop("MIC_SCORE_HEAD", None)
            model.score(px, labels, mask, decoder_input_ids=dec_in, candidates_per_image=G)
            os.environ.pop("MIC_SCORE_HEAD", None)
        return fn

    def alternate(legs, bt):
        for _ in range(2):  # warm-up of every form (buffers keyed on the row counts, GEMM plans)
            for _, fn in legs:
                window(fn, bt, 3)
        meds, allms = {n: [] for n, _ in legs}, {n: [] for n, _ in legs}
        for _ in range(args.alternations):
            for name, fn in legs:
                w = window(fn, bt, args.calls)
                meds[name].append(statistics.median(w))
                allms[name] += w
        return {name: {"ms_per_call": round(statistics.median(allms[name]), 3), "per_alternation_ms": [round(x, 3) for x in meds[name]],
                       "spread_ms": round(max(meds[name]) - min(meds[name]), 3)} for name in meds}

    bench_bt = batches(R, R)
    n_valid = int(bench_bt[0][2].sum())
    if args.trace:
        for head in ("free", "materialised"):
            window(scorer(head), bench_bt, 3 + 4)
        return
    res = {"probe": "score", "rows": R, "seq": T, "valid_rows_of_batch_0": n_valid, "head_free": bool(model.engine.score_head_free(n_valid)),
           "alternations": args.alternations, "calls_per_window": args.calls, "small_debug_model": bool(args.small)}
    case = alternate([("score_free", scorer("free")), ("score_materialised", scorer("materialised")), ("eval_step", lambda b: tr.eval_step(b[4]))], bench_bt)
    spread = max(v["spread_ms"] for v in case.values())
    case["spread_ms"] = spread
    case["free_minus_materialised_ms"] = round(case["score_free"]["ms_per_call"] - case["score_materialised"]["ms_per_call"], 3)
    case["free_minus_eval_step_ms"] = round(case["score_free"]["ms_per_call"] - case["eval_step"]["ms_per_call"], 3)
    res["bench_shape"] = case
    print(f"{R} rows: " + ", ".join(f"{n} {v['ms_per_call']:.3f} ms" for n, v in case.items() if isinstance(v, dict)) +
          f"; free - materialised {case['free_minus_materialised_ms']:+.3f} ms, free - eval_step {case['free_minus_eval_step_ms']:+.3f} ms, spread {spread:.3f} ms")
    G = 16
    g_bt = batches(G * G, G)
    case = alternate([("grouped", scorer("free", G=G)), ("repeated", scorer("free", repeat=G))], g_bt)
    spread = max(v["spread_ms"] for v in case.values())
    gain = case["repeated"]["ms_per_call"] - case["grouped"]["ms_per_call"]
    case.update(spread_ms=spread, gain_ms=round(gain, 3), faster_by_more_than_the_spread=bool(gain > spread))
    res[f"{G}x{G}"] = case
    print(f"{G} images x {G} candidates: grouped {case['grouped']['ms_per_call']:.3f} ms, {G * G} repeated images {case['repeated']['ms_per_call']:.3f} ms; "
          f"gain {gain:+.3f} ms against a spread of {spread:.3f} ms")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
