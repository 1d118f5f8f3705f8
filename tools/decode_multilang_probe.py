"""Four languages per batch: one generate() call per language against ONE grouped call (forced_bos_token_id = the four ids).

Full-size model, batch 256, 4 beams, max_length 64, final_logits_bias[eos] = -1e9 (every search runs its 63 decoder steps, as in
bench.py's beam-4 leg).  Both forms are warmed up (plans allocated, weights folded), then timed alternately in ONE process —
four calls, one grouped call, repeated --reps times, a device synchronisation around every timed window — so that clocks and
allocator state are shared.  Prints captions/s and ms per decoder step of both forms with their spread (a decoder step of the
grouped form carries 4 x the rows), and whether the grouped ids equal the four calls' ids on the timed inputs (bfloat16 runs the
GEMMs of the two forms at different row counts, so low bits of the logits may differ: the agreement rate is reported then).

  python tools/decode_multilang_probe.py [--batch 256] [--reps 3] [--dtype bf16|fp32] [--small] [--json out.json]
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
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--beams", type=int, default=4)
    ap.add_argument("--max-length", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mic_amd import CLIPVisionMBartConfig, FlaxCLIPVisionMBartForConditionalGeneration

    dev = torch.device("cuda:0")
    if args.small:
        cfg = CLIPVisionMBartConfig(mbart_config=dict(vocab_size=5003, d_model=256, decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=512),
                                    clip_vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                            image_size=64, patch_size=16))
    else:
        cfg = CLIPVisionMBartConfig(mbart_config={}, clip_vision_config={})
    model = FlaxCLIPVisionMBartForConditionalGeneration(cfg, seed=0, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32, device=dev)
    st = model.store
    st.f32("flb")[cfg.mbart_config.eos_token_id] = -1e9
    st.refresh_lp()
    V = cfg.mbart_config.vocab_size
    langs = [l if l < V else V - 4 + i for i, l in enumerate((250004, 250008, 250003, 250005))]  # en / fr / de / es
    rng = np.random.default_rng(99)
    img = cfg.clip_vision_config.image_size
    px = torch.from_numpy(np.clip(rng.standard_normal((args.batch, img, img, 3), dtype=np.float32), -1.8, 2.2)).to(dev)
    kw = dict(num_beams=args.beams, max_length=args.max_length)
    steps = args.max_length - 1

    def four_calls():
        outs = [model.generate(px, forced_bos_token_id=l, **kw) for l in langs]
        assert all(o["steps"] == steps for o in outs), [o["steps"] for o in outs]
        return torch.stack([o.sequences for o in outs])

    def grouped_call():
        out = model.generate(px, forced_bos_token_id=langs, **kw)
        assert out["steps"] == [steps] * len(langs), out["steps"]
        return out.sequences

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        seq = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, seq

    for _ in range(2):  # both plans live side by side (two decode plans are kept per model)
        four_calls()
        grouped_call()
    t4, tg, agree = [], [], []
    for _ in range(args.reps):
        dt, s4 = timed(four_calls)
        t4.append(dt)
        dt, sg = timed(grouped_call)
        tg.append(dt)
        agree.append(float((s4 == sg).float().mean().item()))

    n = args.batch * len(langs)

    def figures(ts, decoder_steps):
        med = statistics.median(ts)
        return {"captions_per_s": round(n / med, 1), "captions_per_s_min_max": [round(n / max(ts), 1), round(n / min(ts), 1)],
                "ms_per_decoder_step": round(med / decoder_steps * 1e3, 3),
                "ms_per_decoder_step_min_max": [round(min(ts) / decoder_steps * 1e3, 3), round(max(ts) / decoder_steps * 1e3, 3)],
                "decoder_steps": decoder_steps, "seconds": [round(t, 4) for t in ts]}

    res = {"probe": "decode_multilang", "dtype": args.dtype, "batch": args.batch, "beams": args.beams, "max_length": args.max_length,
           "languages": len(langs), "reps": args.reps, "small_debug_model": bool(args.small),
           "four_calls": figures(t4, len(langs) * steps), "grouped_call": figures(tg, steps),
           "grouped_over_four_calls_captions_per_s": round(statistics.median(t4) / statistics.median(tg), 3),
           "ids_identical": bool(min(agree) == 1.0), "id_agreement_rate_min": round(min(agree), 6)}
    for name in ("four_calls", "grouped_call"):
        f = res[name]
        print(f"{name:>13}: {f['captions_per_s']:9.1f} captions/s (min..max {f['captions_per_s_min_max'][0]}..{f['captions_per_s_min_max'][1]}), "
              f"{f['ms_per_decoder_step']:.3f} ms per decoder step of {f['decoder_steps']} "
              f"(min..max {f['ms_per_decoder_step_min_max'][0]}..{f['ms_per_decoder_step_min_max'][1]})")
    print(f"grouped / four calls (captions/s): {res['grouped_over_four_calls_captions_per_s']:.3f}x; grouped ids "
          + ("identical to the four calls' ids" if res["ids_identical"] else f"agree with the four calls' ids on {res['id_agreement_rate_min']:.4%} of the positions"))
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
