"""The host-side launch sequence of `generate()` calls, mode by mode: every call into libmic_hip.so and every cross-stream
hand-over in issue order (the `Recorder` of tests/util_step_trace.py), with what the calls returned.

A mode (`MODES`) is one model — the small model of util_small.make_pair, 2 decoder layers — and three `generate()` calls on it
with different images: where per-step graphs are on, the first call runs eagerly, the second captures its steps (a capture issues
the step's launches once, which the recorder sees; the replays are graph launches and leave no line) and the third only replays.
The calls of a greedy or beam mode also differ in their forced-BOS ids (step 1 carries them and is never captured).  The calls of
a sampling mode differ in their PRNG keys instead where the plan is keyed by the forced-BOS id (num_return_sequences >= 2): other
ids would be other plans, and no call would replay.

The modes and the run use `generate()`'s public arguments, `final_logits_bias` and the two environment switches only: the same
code drives the commit that recorded tests/golden/generate_trace_parent.json.gz (tests/golden/make_golden_generate_trace.py)
and every later one (tests/test_generate_trace_gpu.py)."""
import gzip
import json
import os

import torch

from util_step_trace import Recorder

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "generate_trace_parent.json.gz")

EOS = 2
SEEDS = (81, 82, 83)           # images of call 1, 2, 3
BOS = (996, 995, 994)          # forced-BOS id of call 1, 2, 3
# a shortlist of the vocabulary: every third id, EOS (= the forced EOS id) and the forced-BOS / language ids
ALLOWED = sorted(set(range(2, 900, 3)) | set(range(990, 1000)))
SAMPLE = dict(do_sample=True, num_beams=1)
WARP = dict(top_k=20, top_p=0.9, temperature=0.7, min_length=3, sample_from_processed_logits=True)


def _calls(common, per_call=None, bos=True):
    """three argument sets: `common`, the call's forced-BOS id (bos=True) and the call's own entries of `per_call`"""
    out = []
    for i in range(3):
        kw = dict(common)
        if bos:
            kw["forced_bos_token_id"] = BOS[i]
        kw.update((per_call or ({},) * 3)[i])
        out.append(kw)
    return out


def _mode(calls, dtype="float32", images=3, eos_bias=None, env=None):
    return dict(calls=calls, dtype=dtype, images=images, eos_bias=eos_bias, env=env or {})


_LANG2 = ({"forced_bos_token_id": [996, 995]}, {"forced_bos_token_id": [994, 996]}, {"forced_bos_token_id": [995, 994]})
_KEYS = ({"prng_key": 11}, {"prng_key": 12}, {"prng_key": 13})

# name -> calls (generate()'s keyword arguments), storage dtype, images per call, EOS entry of final_logits_bias, environment
MODES = {
    # EOS is the argmax from step 2 on: every row has finished long before the poll in front of step 9, which ends the loop
    "greedy_all_finish_early": _mode(_calls(dict(num_beams=1, max_length=20)), eos_bias=30.0),
    "greedy_none_finishes": _mode(_calls(dict(num_beams=1, max_length=20))),
    "greedy_processors": _mode(_calls(dict(num_beams=1, max_length=12, min_length=5, forced_eos_token_id=EOS))),
    "greedy_two_languages": _mode(_calls(dict(num_beams=1, max_length=12), bos=False, per_call=(
        {"forced_bos_token_id": [996, 995]}, {"decoder_start_token_id": [999, 998]},
        {"decoder_start_token_id": [998, 997], "forced_bos_token_id": [994, 996]}))),
    "greedy_shortlist": _mode(_calls(dict(num_beams=1, max_length=12, allowed_token_ids=ALLOWED))),
    "greedy_graphs": _mode(_calls(dict(num_beams=1, max_length=20)), env={"MIC_DECODE_GRAPHS": "1"}),
    "beam4": _mode(_calls(dict(num_beams=4, max_length=12))),                      # top-2K from the head GEMM's partials
    "beam9": _mode(_calls(dict(num_beams=9, max_length=10))),                      # 2K > 16: the streaming top-k
    "beam4_early_stop": _mode(_calls(dict(num_beams=4, max_length=20, decoder_start_token_id=999)), images=4, eos_bias=6.0),
    "beam4_two_languages": _mode(_calls(dict(num_beams=4, max_length=20), bos=False, per_call=_LANG2), eos_bias=0.5),
    "beam4_two_languages_two_best": _mode(_calls(dict(num_beams=4, max_length=20, num_return_sequences=2), bos=False, per_call=_LANG2),
                                          eos_bias=0.5),
    "beam4_shortlist": _mode(_calls(dict(num_beams=4, max_length=12, allowed_token_ids=ALLOWED))),
    # four images in two slices: per-step graphs come on by themselves, the slices' chains are their parallel branches
    "beam4_two_slices": _mode(_calls(dict(num_beams=4, max_length=14), per_call=({}, {"num_return_sequences": 2}, {})), images=4,
                              eos_bias=5.0, env={"MIC_DECODE_SLICES": "2"}),
    "beam4_bf16": _mode(_calls(dict(num_beams=4, max_length=12)), dtype="bfloat16"),
    # the forced EOS at max_length - 1 = 1 beats the per-language BOS of step 1
    "greedy_two_languages_length2": _mode(_calls(dict(num_beams=1, max_length=2), bos=False, per_call=_LANG2)),
    "sample_raw": _mode(_calls(dict(SAMPLE, max_length=12), per_call=_KEYS)),
    "sample_processed": _mode(_calls(dict(SAMPLE, max_length=12, **WARP), per_call=_KEYS)),
    "sample3_raw": _mode(_calls(dict(SAMPLE, max_length=12, num_return_sequences=3), per_call=_KEYS, bos=False)),
    "sample3_processed_graphs": _mode(_calls(dict(SAMPLE, max_length=12, num_return_sequences=3, forced_bos_token_id=996, **WARP),
                                             per_call=_KEYS, bos=False), env={"MIC_DECODE_GRAPHS": "1"}),
}


def _result(out) -> dict:
    """what a call returned, as JSON: token ids, scores (beam search, sampling with num_return_sequences) and step counts (beam search)"""
    res = {"sequences": out.sequences.cpu().tolist()}
    if "scores" in out:
        res["scores"] = out["scores"].float().cpu().tolist()
    if "steps" in out:
        res["steps"] = out["steps"]
    return res


def run_mode(name: str, dev):
    """-> (lines, results): the three `generate()` calls of mode `name` on a fresh model, recorded from the first call on;
    results = `_result` of every call"""
    from mic_amd.params import unflatten_tree
    from util_small import batch, make_pair

    mode = MODES[name]
    env = dict({"MIC_DECODE_GRAPHS": "auto", "MIC_DECODE_SLICES": "auto"}, **mode["env"])
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rc, p, model = make_pair(getattr(torch, mode["dtype"]), dev, gelu="tanh", decoder_ln_eps=1e-6)
        if mode["eos_bias"] is not None:
            p = dict(p)
            flb = p["final_logits_bias"].clone()
            flb[0, rc.eos_token_id] = mode["eos_bias"]
            p["final_logits_bias"] = flb
            model.params = unflatten_tree({k: v.numpy() for k, v in p.items()})
        images = [batch(rc, mode["images"], 12, seed=s)[0].numpy() for s in SEEDS]
        torch.cuda.synchronize()
        results = []
        with Recorder() as rec:
            for px, kw in zip(images, mode["calls"]):
                results.append(_result(model.generate(px, **kw)))
        torch.cuda.synchronize()
        model.release_decode_plans()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return rec.events, results


def pack(runs: dict) -> dict:
    """{mode: (lines, results)} -> the fixture's layout: one table of distinct lines, a list of indices into it per mode"""
    table, index = [], {}
    out = {"lines": table, "modes": {}}
    for name, (lines, results) in runs.items():
        seq = []
        for ln in lines:
            if ln not in index:
                index[ln] = len(table)
                table.append(ln)
            seq.append(index[ln])
        out["modes"][name] = {"seq": seq, "calls": results}
    return out


def load_fixture(path: str = FIXTURE) -> dict:
    """-> {mode: (lines, results)}"""
    with gzip.open(path, "rt") as f:
        fx = json.load(f)
    return {name: ([fx["lines"][i] for i in m["seq"]], m["calls"]) for name, m in fx["modes"].items()}
