"""Recorder of the host-side launch sequence of Trainer steps: every call into libmic_hip.so and every cross-stream hand-over
(`torch.cuda.Event.record`, `Stream.wait_event`, `Stream.wait_stream`), in issue order, as one line of text per call.

`Recorder` swaps the loaded library in `mic_amd._lib` for a proxy that writes the call down and calls through.  Of a call it keeps
the entry name, the integer and floating-point arguments by value, pointer arguments as null (`0`) or non-null (`p`) and the
stream (the last pointer argument of every launching entry) as `s<k>`, k numbered by first appearance.  Structure arguments
(`mic_gemm_args`, the items of the grouped entries, the fp8 emission descriptors) are written out field by field under the same
rules, zero fields left out: for the GEMM entries that is M, N, K, the dtypes and fp8 formats, the k-major flags, act, dact,
accumulate, split_k, k_valid and the leading dimensions / seeds / strides per problem.  Events are `e<k>`, numbered by first
appearance as well (the recorder keeps them alive, so an address is never counted twice).

The modes (`MODES`) and the run (`run_mode`) use public constructor arguments and environment switches only: the same code
drives the commit that recorded tests/golden/step_trace_parent.json.gz (tests/golden/make_golden_step_trace.py) and every later
one (tests/test_step_trace_gpu.py)."""
import ctypes as C
import gzip
import json
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "step_trace_parent.json.gz")

# the 256-wide small model of tests/test_fp8_gpu.py: d and Vpad in whole 128-byte fragments, so the fp8 head is "all"
WIDE = dict(d_model=256, d_ffn=512, d_heads=4, v_hidden=256, v_ffn=512, v_heads=4)
FP8 = dict(gemm_dtype="fp8", bucket_mb=0.25)
B, T, TRAIN_STEPS = 3, 12, 4
# name -> (storage dtype, model overrides, Trainer arguments, environment)
MODES = {
    "bf16": ("bfloat16", {}, {}, {}),
    "bf16_no_overlap": ("bfloat16", {}, dict(overlap_optimizer=False), {}),
    "bf16_accumulate2": ("bfloat16", {}, dict(accumulate_steps=2), {}),
    "bf16_padded_rows": ("bfloat16", {}, dict(pack_rows=False), {}),
    "f32": ("float32", {}, {}, {}),
    "fp8": ("bfloat16", WIDE, FP8, {}),
    "fp8_unfused": ("bfloat16", WIDE, FP8, {"MIC_FP8_FUSED": "0"}),
    "fp8_w8_sync": ("bfloat16", WIDE, FP8, {"MIC_FP8_W8_ASYNC": "0"}),
    "fp8_current": ("bfloat16", WIDE, dict(FP8, fp8_scaling="current"), {}),
    "fp8_head_bwd": ("bfloat16", WIDE, dict(FP8, fp8_head="bwd"), {}),
    "fp8_no_overlap": ("bfloat16", WIDE, dict(FP8, overlap_optimizer=False), {}),
}

# array arguments: entry -> position of the item count (every other structure argument is a single one passed by reference)
_COUNT_ARG = {"mic_gemm_grouped": 1, "mic_fp8_amax": 1, "mic_fp8_quantize": 1, "mic_ln_param_grads": 1, "mic_colsum_q8_grouped": 1,
              "mic_colsum_grouped": 2, "mic_beam_step_groups": 1, "mic_image_transform": 1, "mic_gemm_plan": 1}
# once per process, whoever asks first (`ops.cu_masked_stream`): not part of a step's sequence
_NOT_RECORDED = ("mic_stream_create_cu_masked", "mic_stream_destroy", "mic_last_error")
_INTS = (C.c_int, C.c_uint32, C.c_int64, C.c_longlong)
_FLOATS = (C.c_float, C.c_double)


def _num(v):
    return "%.9g" % v if isinstance(v, float) else str(int(v))


def _struct(s) -> str:
    out = []
    for name, ty in s._fields_:
        v = getattr(s, name)
        if ty is C.c_void_p:
            if v:
                out.append(name + "=p")
        elif v:
            out.append(f"{name}={_num(v)}")
    return "{" + ",".join(out) + "}"


class Recorder:
    """with Recorder() as rec: ...; rec.events is the list of lines"""

    def __init__(self):
        self.events, self._streams, self._events, self._keep, self._depth = [], {}, {}, [], 0

    def _s(self, handle) -> str:
        h = int(handle or 0)
        return "s%d" % self._streams.setdefault(h, len(self._streams))

    def _e(self, ev) -> str:
        k = id(ev)
        if k not in self._events:
            self._events[k] = len(self._events)
            self._keep.append(ev)
        return "e%d" % self._events[k]

    def _call(self, name, sig, args) -> str:
        out = []
        for i, (ty, v) in enumerate(zip(sig, args)):
            if ty in _INTS:
                out.append(str(int(v)))
            elif ty in _FLOATS:
                out.append(_num(float(v)))
            elif ty is C.c_void_p:
                out.append(self._s(v) if i == len(sig) - 1 else ("p" if v else "0"))
            elif v is None:
                out.append("0")
            elif hasattr(v, "_obj"):  # byref(structure)
                out.append(_struct(v._obj) if hasattr(v._obj, "_fields_") else "p")
            elif name in _COUNT_ARG and hasattr(v, "__getitem__") and hasattr(getattr(v, "_type_", None), "_fields_"):
                out.append("[" + ",".join(_struct(v[j]) for j in range(int(args[_COUNT_ARG[name]]))) + "]")
            else:
                out.append("p")
        return f"{name}({','.join(out)})"

    def __enter__(self):
        from mic_amd import _lib as L

        real, rec = L.lib(), self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if not name.startswith("mic_") or name in _NOT_RECORDED:
                    return fn
                sig = L._SIGS[name][0]

                def call(*args):
                    rec.events.append(rec._call(name, sig, args))
                    return fn(*args)
                setattr(self, name, call)
                return call

        self._real, self._L = real, L
        L._lib = Proxy()
        E, S = torch.cuda.Event, torch.cuda.Stream
        self._orig = (E.record, S.wait_event, S.wait_stream)
        o_record, o_wait_event, o_wait_stream = self._orig

        def nested(line, fn, *a):
            if rec._depth == 0:
                rec.events.append(line)
            rec._depth += 1
            try:
                return fn(*a)
            finally:
                rec._depth -= 1

        def record(ev, stream=None):
            st = stream if stream is not None else torch.cuda.current_stream()
            return nested(f"event_record({rec._e(ev)},{rec._s(st.cuda_stream)})" if rec._depth == 0 else "", o_record, ev, st)

        def wait_event(st, ev):
            return nested(f"wait_event({rec._s(st.cuda_stream)},{rec._e(ev)})" if rec._depth == 0 else "", o_wait_event, st, ev)

        def wait_stream(st, other):  # (torch: an event recorded on `other` and waited for — one line here)
            return nested(f"wait_stream({rec._s(st.cuda_stream)},{rec._s(other.cuda_stream)})", o_wait_stream, st, other)

        E.record, S.wait_event, S.wait_stream = record, wait_event, wait_stream
        return self

    def __exit__(self, *exc):
        E, S = torch.cuda.Event, torch.cuda.Stream
        E.record, S.wait_event, S.wait_stream = self._orig
        self._L._lib = self._real
        return False


def run_mode(name: str, dev):
    """-> (lines, losses): TRAIN_STEPS `train_step` calls and one `eval_step` of a fresh Trainer in mode `name`, recorded from the
    Trainer's construction on; losses = the value every one of those calls returned"""
    from mic_amd import Trainer, create_learning_rate_fn
    from util_small import batch, make_pair

    dtype, over, kw, env = MODES[name]
    keep = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rc, _, model = make_pair(getattr(torch, dtype), dev, gelu="tanh", decoder_ln_eps=1e-6, dropout=0.1, **over)
        px, labels, mask, dec_in = batch(rc, B, T, seed=9)
        b = {"pixel_values": px.numpy(), "input_ids": labels.numpy(), "attention_mask": mask.numpy(), "decoder_input_ids": dec_in.numpy()}
        torch.cuda.synchronize()
        with Recorder() as rec:
            tr = Trainer(model, create_learning_rate_fn(64, 2, 4, 2, 2e-3), **kw)
            losses = [float(tr.train_step(b)["loss"]) for _ in range(TRAIN_STEPS)]
            losses.append(float(tr.eval_step(b)["loss"]))
        torch.cuda.synchronize()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return rec.events, losses


def pack(runs: dict) -> dict:
    """{mode: (lines, losses)} -> the fixture's layout: one table of distinct lines, a list of indices into it per mode"""
    table, index = [], {}
    out = {"lines": table, "modes": {}}
    for name, (lines, losses) in runs.items():
        seq = []
        for ln in lines:
            if ln not in index:
                index[ln] = len(table)
                table.append(ln)
            seq.append(index[ln])
        out["modes"][name] = {"seq": seq, "losses": losses}
    return out


def load_fixture(path: str = FIXTURE) -> dict:
    """-> {mode: (lines, losses)}"""
    with gzip.open(path, "rt") as f:
        fx = json.load(f)
    return {name: ([fx["lines"][i] for i in m["seq"]], m["losses"]) for name, m in fx["modes"].items()}
