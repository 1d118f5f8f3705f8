"""generate(do_sample=True, num_return_sequences=N) against N separate sampling calls: what N sampled captions per image cost either way.

Full-size model, bfloat16, max_length 64, final_logits_bias[eos] = -1e9 (no draw ends early: every chain runs its 63 decoder steps),
N = 4 draws per image.  Forms, each in the reference's raw-logits mode and in the processed mode with top_k = 50:
  separate   N calls generate(do_sample=True, prng_key=keys[n]): N encoder passes, N chains of `batch` rows (`_sample`: per-call
             allocation, a host sync per step, mic_sample_rows);
  grouped    one call generate(do_sample=True, num_return_sequences=N): one encoder pass, one chain of batch * N rows from a decode
             plan (mic_sample_rows_keyed).
All forms are warmed up, then timed alternately in ONE process, --reps rounds, a device synchronisation around every timed window.
Prints ms per decoder step (of the form's whole work: the N chains of `separate` together) and captions/s per form with their
spread, and grouped over separate.  The yardstick is `separate` on the same commit in the same process.

  python tools/sample_probe.py [--batch 64] [--draws 4] [--reps 3] [--modes raw,processed] [--small] [--json out.json]

The sampling kernels' own times: run the probe with --reps 1 under `rocprofv3 --kernel-trace --stats` (a run of its own) and set
sample_rows_keyed_kernel / sample_rows_kernel against one pass over rows x V logits at the HBM peak (the JSON line carries those bytes).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0  # MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--draws", type=int, default=4)
    ap.add_argument("--max-length", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="raw,processed")
    ap.add_argument("--top-k", type=int, default=50)
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mic_amd import CLIPVisionMBartConfig, FlaxCLIPVisionMBartForConditionalGeneration, prng

    dev = torch.device("cuda:0")
    if args.small:
        cfg = CLIPVisionMBartConfig(mbart_config=dict(vocab_size=5003, d_model=256, decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=512),
                                    clip_vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                            image_size=64, patch_size=16))
    else:
        cfg = CLIPVisionMBartConfig(mbart_config={}, clip_vision_config={})
    model = FlaxCLIPVisionMBartForConditionalGeneration(cfg, seed=0, dtype=torch.bfloat16, device=dev)
    st = model.store
    eos, pad = cfg.mbart_config.eos_token_id, cfg.mbart_config.pad_token_id
    st.f32("flb")[eos] = -1e9
    st.refresh_lp()
    V = cfg.mbart_config.vocab_size
    rng = np.random.default_rng(99)
    img = cfg.clip_vision_config.image_size
    px = torch.from_numpy(np.clip(rng.standard_normal((args.batch, img, img, 3), dtype=np.float32), -1.8, 2.2)).to(dev)
    N, steps = args.draws, args.max_length - 1
    keys = prng.split(prng.prng_key(1), N)
    modes = [m for m in args.modes.split(",") if m]
    kw = {"raw": dict(), "processed": dict(sample_from_processed_logits=True, top_k=args.top_k, top_p=1.0, temperature=1.0)}
    base = dict(do_sample=True, num_beams=1, max_length=args.max_length)

    def separate(mode):
        return torch.cat([model.generate(px, prng_key=keys[n], **base, **kw[mode]).sequences for n in range(N)])

    def grouped(mode):
        return model.generate(px, prng_key=1, num_return_sequences=N, **base, **kw[mode]).sequences

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*a)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    forms = [(f, m) for m in modes for f in ("separate", "grouped")]
    fns = {"separate": separate, "grouped": grouped}
    for _ in range(2):
        for f, m in forms:
            fns[f](m)
    times = {fm: [] for fm in forms}
    lengths = {}
    for _ in range(args.reps):
        for f, m in forms:
            dt, seq = timed(fns[f], m)
            times[(f, m)].append(dt)
            lengths[(f, m)] = float((seq[:, 1:] != pad).sum(1).float().mean().item())

    def figures(ts):
        med = statistics.median(ts)
        return {"captions_per_s": round(args.batch * N / med, 1),
                "captions_per_s_min_max": [round(args.batch * N / max(ts), 1), round(args.batch * N / min(ts), 1)],
                "ms_per_decoder_step": round(med / steps * 1e3, 3),
                "ms_per_decoder_step_min_max": [round(min(ts) / steps * 1e3, 3), round(max(ts) / steps * 1e3, 3)],
                "seconds": [round(t, 4) for t in ts]}

    rows = args.batch * N
    res = {"probe": "sample", "dtype": "bf16", "batch": args.batch, "draws": N, "max_length": args.max_length, "decoder_steps": steps,
           "reps": args.reps, "small_debug_model": bool(args.small), "vocab_size": V, "top_k": args.top_k,
           "forms": {f"{m}_{f}": figures(times[(f, m)]) for f, m in forms},
           "mean_caption_tokens": {f"{m}_{f}": round(lengths[(f, m)], 2) for f, m in forms},
           "one_pass_over_the_logits": {"rows": rows, "bytes": rows * V * 2, "us_at_hbm_peak": round(rows * V * 2 / (HBM_PEAK_TBS * 1e12) * 1e6, 2)}}
    for m in modes:
        a, b = res["forms"][f"{m}_separate"], res["forms"][f"{m}_grouped"]
        b["speedup_over_separate"] = round(statistics.median(times[("separate", m)]) / statistics.median(times[("grouped", m)]), 3)
        for name, r in (("separate", a), ("grouped", b)):
            print(f"{m:>10} {name:>9}: {r['ms_per_decoder_step']:.3f} ms per decoder step (min..max {r['ms_per_decoder_step_min_max'][0]}.."
                  f"{r['ms_per_decoder_step_min_max'][1]}), {r['captions_per_s']:8.1f} captions/s (min..max {r['captions_per_s_min_max'][0]}.."
                  f"{r['captions_per_s_min_max'][1]})")
        print(f"{m:>10}: grouped is {b['speedup_over_separate']:.3f}x separate")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
