"""What packed decoder rows buy at seq_len 128: `Trainer.train_step` on packed rows against the same step on padded rows.

Full-size model, batch 64, T = 128, device-resident batches with the collate extras (bench.py's train leg), batches from
`bench.synth_batch`: ragged captions (n ~ U{8..T-2} tokens, about 54 % of the B*T positions valid) and dense ones (`dense=True`:
every caption fills its row; there is nothing to pack and the Trainer runs the padded step either way — the leg shows that the
switch itself costs nothing).  bf16 and `gemm_dtype="fp8"`, one Trainer each, built one after the other in ONE process (a second
live Trainer shifts how the streams map onto hardware queues, `ops.role_stream`).  The padded leg is that same Trainer with
`pack_rows` switched off: `_prep` then takes the path of `Trainer(pack_rows=False)` launch for launch — which is what a Trainer did at
this length before the tiled attention kernels took packed rows.  After warm-up of both forms the two are timed alternately with
device events, one event between any two calls.

Verdict per storage / caption kind: packed faster than padded in EVERY alternation by more than the spread (the larger of the two
forms' max - min over the alternations' window means); dense: packed not slower than padded by more than that spread.

  python tools/seq128_probe.py [--batch 64] [--seq 128] [--steps 30] [--alternations 3] [--gemm-dtypes bf16,fp8] [--small] [--json out.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seq", type=int, default=128)
    ap.add_argument("--steps", type=int, default=30, help="train steps per timed window (30: about a second per window)")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--gemm-dtypes", default="bf16,fp8")
    ap.add_argument("--small", action="store_true", help="reduced model (debugging the probe itself; not a measurement)")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    assert args.alternations >= 3 and args.steps >= 2

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
    B, T = args.batch, args.seq
    V, img = cfg.mbart_config.vocab_size, cfg.clip_vision_config.image_size

    def batches_of(dense):
        out, share = [], []
        for i in range(2):
            b = bench.synth_batch(B, T, V, img, 1234 + i, dense=dense)
            share.append(float(b["attention_mask"].mean()))
            db = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
            idx, rl = loss_rows(b["attention_mask"], b["input_ids"])
            db["loss_rows"] = (torch.from_numpy(idx).to(dev), torch.from_numpy(rl).to(dev))
            pk = packed_rows(b["attention_mask"], b["decoder_input_ids"])
            if pk is not None:
                db["packed_rows"] = tuple(torch.from_numpy(t).to(dev) for t in pk)
            out.append(db)
        return out, sum(share) / len(share)

    kinds = {"ragged": batches_of(False), "dense": batches_of(True)}
    r3 = lambda xs: [round(x, 3) for x in xs]  # noqa: E731
    res = {"probe": "seq128", "batch": B, "seq": T, "steps_per_window": args.steps, "alternations": args.alternations,
           "small_debug_model": bool(args.small), "valid_row_share": {k: round(v[1], 4) for k, v in kinds.items()}}
    for gd in args.gemm_dtypes.split(","):
        model = FlaxCLIPVisionMBartForConditionalGeneration(cfg, seed=0, dtype=torch.bfloat16, device=dev)
        lr_fn = create_learning_rate_fn(train_ds_size=10_000_000, train_batch_size=B, num_train_epochs=7, num_warmup_steps=1000, learning_rate=5e-5)
        tr = Trainer(model, lr_fn, seed=42, **({} if gd == "bf16" else dict(gemm_dtype=gd)))
        assert tr.pack_rows, "MIC_PACK_ROWS=0 in the environment: nothing to compare"

        def window(batches, pack):
            """args.steps train_step calls, an event between any two: ms of each call on the device"""
            tr.pack_rows = pack
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
            ev[0].record()
            for i in range(args.steps):
                tr.train_step(batches[i % 2])
                ev[i + 1].record()
            torch.cuda.synchronize()
            return [ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)], tr._pack is not None

        res[gd] = {}
        for kind, (batches, share) in kinds.items():
            for pack in (True, False, True, False):  # warm-up of both forms (buffers, plans, fp8 scale histories)
                window(batches, pack)
            packed, padded = [], []
            for _ in range(args.alternations):
                w, was_packed = window(batches, True)
                assert was_packed == (kind == "ragged"), (kind, was_packed)
                packed.append(statistics.mean(w))
                w, was_packed = window(batches, False)
                assert not was_packed
                padded.append(statistics.mean(w))
            spread = max(max(packed) - min(packed), max(padded) - min(padded))
            gain = [b - a for a, b in zip(packed, padded)]
            ok = all(g > spread for g in gain) if kind == "ragged" else all(g > -spread for g in gain)
            res[gd][kind] = {"ms_per_step_packed": r3(packed), "ms_per_step_padded": r3(padded), "spread_ms": round(spread, 3),
                             "padded_minus_packed_ms": r3(gain), "rows_really_packed": kind == "ragged", "valid_row_share": round(share, 4),
                             "images_per_s_packed": round(B / statistics.median(packed) * 1e3, 1),
                             "images_per_s_padded": round(B / statistics.median(padded) * 1e3, 1), "condition_met": bool(ok)}
            print(f"{gd} {kind} (valid rows {share:.3f}): packed {r3(packed)} ms/step, padded {r3(padded)} ms/step, spread {spread:.3f} ms -> "
                  + (("packed faster in every alternation by more than the spread" if kind == "ragged" else "packed not slower beyond the spread")
                     if ok else "CONDITION NOT MET"))
        del tr, model
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
