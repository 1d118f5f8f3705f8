"""generate(allowed_token_ids=A) against the plain call: what the decoder step costs when the LM head and the top-k run over a
shortlist of the vocabulary.

Full-size model, bfloat16, batch 256, 4 beams, max_length 64, final_logits_bias[eos] = -1e9 (every search runs its 63 decoder steps,
as in bench.py's beam-4 leg).  Forms: the plain call and one call per shortlist size (8 192, 32 768, 65 536 random ids + EOS).  All
forms are warmed up (plans allocated — the probe keeps one decode plan per form alive —, weights folded, rows gathered), then timed
alternately in ONE process, --reps rounds, a device synchronisation around every timed window.  Prints ms per decoder step and
captions/s per form with their spread, the speed-up over the plain call, and what building a shortlist costs (allocation + gather of
len(A) embedding rows, synchronised; the in-place re-gather after a weight change alone).

--plain-only times the plain call alone (the same windows): run it alternately from two checkouts to compare their plain paths.

  python tools/shortlist_probe.py [--batch 256] [--reps 3] [--sizes 8192,32768,65536] [--plain-only] [--small] [--json out.json]
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
    ap.add_argument("--sizes", default="8192,32768,65536")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    from mic_amd import CLIPVisionMBartConfig, FlaxCLIPVisionMBartForConditionalGeneration
    from mic_amd import generation_clip_vision_utils as G

    dev = torch.device("cuda:0")
    if args.small:
        cfg = CLIPVisionMBartConfig(mbart_config=dict(vocab_size=5003, d_model=256, decoder_layers=2, decoder_attention_heads=4, decoder_ffn_dim=512),
                                    clip_vision_config=dict(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                                                            image_size=64, patch_size=16))
    else:
        cfg = CLIPVisionMBartConfig(mbart_config={}, clip_vision_config={})
    model = FlaxCLIPVisionMBartForConditionalGeneration(cfg, seed=0, dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32, device=dev)
    st = model.store
    eos = cfg.mbart_config.eos_token_id
    st.f32("flb")[eos] = -1e9
    st.refresh_lp()
    V = cfg.mbart_config.vocab_size
    rng = np.random.default_rng(99)
    img = cfg.clip_vision_config.image_size
    px = torch.from_numpy(np.clip(rng.standard_normal((args.batch, img, img, 3), dtype=np.float32), -1.8, 2.2)).to(dev)
    kw = dict(num_beams=args.beams, max_length=args.max_length)
    steps = args.max_length - 1

    sizes = [] if args.plain_only else [min(int(s), V - 1) for s in args.sizes.split(",") if s]
    sets = {n: np.unique(np.concatenate([rng.choice(V, size=n, replace=False), [eos]])).astype(np.int32) for n in sizes}
    forms = ["plain"] + [f"shortlist_{n}" for n in sizes]
    G._MAX_PLANS = max(G._MAX_PLANS, len(forms))          # one warm plan (KV cache, buffers) per form, side by side
    if sizes:
        G._MAX_SHORTLISTS = max(G._MAX_SHORTLISTS, len(sizes))

    def call(form):
        extra = {} if form == "plain" else {"allowed_token_ids": sets[int(form.split("_")[1])]}
        out = model.generate(px, **kw, **extra)
        assert out["steps"] == steps, (form, out["steps"])
        return out.sequences

    def timed(fn, *a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn(*a)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    build = {}
    for n in sizes:  # what a distinct set costs once: allocation + gather; and the in-place re-gather after a weight change
        from mic_amd.engine import Shortlist

        def fresh():
            sl = Shortlist(model.engine, sets[n], (n, "probe"))
            sl.refresh()
            return sl

        fresh()  # (first use of the gather kernels)
        t_new, sl = timed(fresh)
        sl.version = None
        t_again, _ = timed(sl.refresh)
        build[n] = {"build_ms": round(t_new * 1e3, 3), "regather_ms": round(t_again * 1e3, 3), "ids": int(sets[n].size)}
        del sl

    for _ in range(2):
        for f in forms:
            call(f)
    times = {f: [] for f in forms}
    inside = {}
    for _ in range(args.reps):
        for f in forms:
            dt, seq = timed(call, f)
            times[f].append(dt)
            if f != "plain":
                ids = sets[int(f.split("_")[1])]
                inside[f] = bool(np.isin(seq[:, 1:].cpu().numpy(), np.concatenate([ids, [cfg.mbart_config.pad_token_id]])).all())

    def figures(ts):
        med = statistics.median(ts)
        return {"captions_per_s": round(args.batch / med, 1), "captions_per_s_min_max": [round(args.batch / max(ts), 1), round(args.batch / min(ts), 1)],
                "ms_per_decoder_step": round(med / steps * 1e3, 3),
                "ms_per_decoder_step_min_max": [round(min(ts) / steps * 1e3, 3), round(max(ts) / steps * 1e3, 3)],
                "seconds": [round(t, 4) for t in ts]}

    res = {"probe": "shortlist", "dtype": args.dtype, "batch": args.batch, "beams": args.beams, "max_length": args.max_length, "decoder_steps": steps,
           "reps": args.reps, "small_debug_model": bool(args.small), "vocab_size": V, "forms": {f: figures(times[f]) for f in forms},
           "shortlist_build": build, "emitted_ids_inside_the_set": inside}
    base = statistics.median(times["plain"])
    for f in forms:
        r = res["forms"][f]
        r["speedup_over_plain"] = round(base / statistics.median(times[f]), 3)
        print(f"{f:>16}: {r['ms_per_decoder_step']:.3f} ms per decoder step (min..max {r['ms_per_decoder_step_min_max'][0]}..{r['ms_per_decoder_step_min_max'][1]}), "
              f"{r['captions_per_s']:8.1f} captions/s (min..max {r['captions_per_s_min_max'][0]}..{r['captions_per_s_min_max'][1]}), "
              f"{r['speedup_over_plain']:.3f}x the plain call")
    for n, b in build.items():
        print(f"shortlist of {b['ids']} ids: build {b['build_ms']:.3f} ms (allocation + gather), re-gather in place {b['regather_ms']:.3f} ms")
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
