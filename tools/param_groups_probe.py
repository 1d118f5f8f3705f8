"""What parameter groups (`Trainer(param_groups=...)`) cost or save at the bench workload: the plain `Trainer.train_step` against the
step with `NO_DECAY` only (and, to attribute its distance, the plain step without the tied embedding's row split), with the image
tower frozen and its backward still run, and with the frozen tower's backward skipped.

Full-size model, bf16, batch 64, seq 64, ragged captions, device-resident batches with the collate extras (bench.py's train leg).
ONE process and ONE Trainer (a second Trainer in a process shifts how its streams map onto hardware queues, `ops.role_stream`): it
is built with `param_groups=[dict(match=ENCODER, frozen=True)]` and switched between the forms by writing the state the
constructor derives from the option (`mode()` below) — in the plain form `train_step` takes the path of a Trainer built without the
keyword, launch for launch.  After warm-up of all forms they are timed alternately with device events, one event between any two
calls (`train_step` joins its side streams into the caller's stream before it returns, so the events see the optimizer too).

What to expect: NO_DECAY only differs from plain by the tied embedding's row split being off (its 1 GB of optimizer passes wait for
the end of backward instead of running beside it) and by the grouped kernel; a frozen tower with full backward saves the ViT's
optimizer passes only; skipping the backward removes the ViT's layer backward and its weight-gradient GEMMs from the step.

  python tools/param_groups_probe.py [--batch 64] [--steps 8] [--alternations 3] [--small] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# plain_no_row_split is not a form a user can ask for by this route: the plain step with the tied embedding's row split off (what
# MIC_OPT_SPLIT_SHARED=0 does), there to attribute the distance between no_decay and plain
FORMS = ("plain", "plain_no_row_split", "no_decay", "frozen_full_backward", "frozen_skipped_backward")


def main():
    ap = argparse.ArgumentParser()
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
    from mic_amd.train import ENCODER, NO_DECAY, param_group_table

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
    frozen_groups = [dict(match=ENCODER, frozen=True)]
    tr = Trainer(model, lr_fn, seed=42, weight_decay=0.01, param_groups=frozen_groups)
    r, st = tr.reducer, model.store
    assert tr.overlap_optimizer and r.on_ready is not None and not tr._split_shared and tr._encoder_frozen and tr.skip_frozen_backward
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

    # the forms of everything Trainer.__init__ derives from param_groups
    sb, se, width = tr._sh
    assert (se - sb) % width == 0
    nd_runs = param_group_table(st, [dict(match=NO_DECAY, weight_decay=0.0)], tr.wd)
    grouped_when = list(r.ready_when)
    plain_when = ["next" if (b < se and e > sb) else "exchanged" for (b, e) in tr.buckets]
    row_flag = torch.zeros((se - sb) // width, dtype=torch.uint8, device=dev)
    state = {
        "plain": dict(_groups=None, _group_runs=None, _encoder_frozen=False, skip_frozen_backward=True, _split_shared=True, _row_flag=row_flag),
        "plain_no_row_split": dict(_groups=None, _group_runs=None, _encoder_frozen=False, skip_frozen_backward=True, _split_shared=False,
                                   _row_flag=None),
        "no_decay": dict(_groups=ops.AdamwRuns(nd_runs, dev), _group_runs=nd_runs, _encoder_frozen=False, skip_frozen_backward=True,
                         _split_shared=False, _row_flag=None),
        "frozen_full_backward": dict(_groups=tr._groups, _group_runs=tr._group_runs, _encoder_frozen=True, skip_frozen_backward=False,
                                     _split_shared=False, _row_flag=None),
        "frozen_skipped_backward": dict(_groups=tr._groups, _group_runs=tr._group_runs, _encoder_frozen=True, skip_frozen_backward=True,
                                        _split_shared=False, _row_flag=None),
    }

    def mode(form):
        for k, v in state[form].items():
            setattr(tr, k, v)
        r.ready_when = list(plain_when if form == "plain" else grouped_when)

    def window(n_calls):
        """n_calls train_step calls, an event between any two: ms of each call on the device"""
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_calls + 1)]
        ev[0].record()
        for i in range(n_calls):
            tr.train_step(batches[i % 2])
            ev[i + 1].record()
        torch.cuda.synchronize()
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(n_calls)]

    for form in FORMS + FORMS:  # warm-up of every form (buffers, plans, the k-major embedding copy)
        mode(form)
        window(K)
    ms = {f: [] for f in FORMS}
    for _ in range(args.alternations):
        for form in FORMS:
            mode(form)
            ms[form].append(window(K))

    med = {f: statistics.median([x for w in ms[f] for x in w]) for f in FORMS}
    tot = {f: [sum(w) for w in ms[f]] for f in FORMS}
    spread = {f: (max(tot[f]) - min(tot[f])) / K for f in FORMS}
    worst = max(spread.values())
    r3 = lambda xs: [round(x, 3) for x in xs]  # noqa: E731
    res = {"probe": "param_groups", "batch": B, "seq": T, "steps_per_window": K, "alternations": args.alternations,
           "small_debug_model": bool(args.small), "buckets": len(tr.buckets), "elements": int(st.numel),
           "runs_no_decay": len(nd_runs), "runs_frozen": len(tr._group_runs),
           "frozen_elements": int(sum(e - b for (b, e, _, _, f) in tr._group_runs if f)),
           "ms_per_step": {f: round(med[f], 3) for f in FORMS}, "images_per_s": {f: round(B / med[f] * 1e3, 1) for f in FORMS},
           "ms_windows": {f: r3(tot[f]) for f in FORMS}, "spread_ms_per_step": {f: round(spread[f], 3) for f in FORMS},
           "no_decay_minus_plain_ms": round(med["no_decay"] - med["plain"], 3),
           "no_row_split_minus_plain_ms": round(med["plain_no_row_split"] - med["plain"], 3),
           "no_decay_minus_no_row_split_ms": round(med["no_decay"] - med["plain_no_row_split"], 3),
           "frozen_full_minus_plain_ms": round(med["frozen_full_backward"] - med["plain"], 3),
           "skipped_minus_full_ms": round(med["frozen_skipped_backward"] - med["frozen_full_backward"], 3),
           "skipping_is_faster_beyond_spread": bool(med["frozen_full_backward"] - med["frozen_skipped_backward"] > worst)}
    for f in FORMS:
        print(f"{f:<26} {med[f]:8.3f} ms/step  {B / med[f] * 1e3:8.1f} images/s  spread {spread[f]:.3f} ms/step  windows {r3(tot[f])}")
    print(f"no_decay - plain {res['no_decay_minus_plain_ms']:+.3f} ms, of which the row split being off {res['no_row_split_minus_plain_ms']:+.3f} ms "
          f"and the grouped kernel {res['no_decay_minus_no_row_split_ms']:+.3f} ms; frozen (full backward) - plain {res['frozen_full_minus_plain_ms']:+.3f} ms; "
          f"skipped - full {res['skipped_minus_full_ms']:+.3f} ms -> skipping is "
          + ("faster beyond the spread" if res["skipping_is_faster_beyond_spread"] else "NOT faster beyond the spread"))
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(res, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
