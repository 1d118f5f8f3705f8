"""The training attention's host side, without a GPU: every refusal of the seven entry points (each returns before any HIP call, so
stand-in addresses are never dereferenced), and the engine's choice of entry point at its attention call sites."""
import ctypes as C
import inspect
import os
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

MIC_EINVAL = -1
BF16, F32, E4M3, E5M2 = 0, 1, 0, 1
ADDR = 0x1000  # a stand-in address: every case below is refused before anything reads it

FWD = "dtype B H Tq Tk q ldq k ldk v ldv out ldo key_mask causal lse stream"
BWD = "dtype B H Tq Tk q ldq k ldk v ldv out ldo dout lddo lse key_mask causal dq lddq dk lddk dv lddv stream"
FWD_PACKED = "dtype B H Tq Tk q_off q_len kv_packed q ldq k ldk v ldv out ldo causal lse stream"
BWD_PACKED = "dtype B H Tq Tk q_off q_len kv_packed q ldq k ldk v ldv out ldo dout lddo lse causal dq lddq dk lddk dv lddv stream"
BWD_Q8 = "B H Tq Tk q_off q_len kv_packed q ldq k ldk v ldv out ldo dout lddo lse key_mask causal dq8 dk8 dv8 stream"
ARGS = {"mic_attn_fwd": FWD, "mic_attn_bwd": BWD, "mic_attn_fwd_packed": FWD_PACKED, "mic_attn_bwd_packed": BWD_PACKED,
        "mic_attn_fwd_packed_tiled": FWD_PACKED, "mic_attn_bwd_packed_tiled": BWD_PACKED, "mic_attn_bwd_q8": BWD_Q8}
ONE_TILE = ("mic_attn_fwd_packed", "mic_attn_bwd_packed", "mic_attn_bwd_q8")
TILED_PACKED = ("mic_attn_fwd_packed_tiled", "mic_attn_bwd_packed_tiled")
FWD_POINTERS, BWD_POINTERS = ("q", "k", "v", "out"), ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv")
FWD_STRIDES, BWD_STRIDES = ("ldq", "ldk", "ldv"), ("ldq", "ldk", "ldv", "ldo", "lddo")


def _fp8_out(**kw):
    """(q, ldq, state, amax_next, fmt) of an `Fp8Out` descriptor; amax_next may be null"""
    return dict(dict(q=ADDR, ldq=128, state=ADDR, amax_next=None, fmt=E5M2), **kw)


def _good(name):
    """arguments of a call that every check lets through (never sent as they are: each case breaks exactly one of them)"""
    a = {n: ADDR for n in ARGS[name].split() if n in BWD_POINTERS}
    a.update(dtype=BF16, B=2, H=2, Tq=16, Tk=16, causal=0, kv_packed=0, key_mask=None, stream=None)
    a.update({n: 128 for n in ARGS[name].split() if n.startswith("ld")})
    if "packed" in name:
        a.update(q_off=ADDR, q_len=ADDR)
    if name == "mic_attn_bwd_q8":  # dense rows by default (q_off == q_len == NULL)
        a.update(q_off=None, q_len=None, dq8=_fp8_out(), dk8=_fp8_out(), dv8=ADDR)
    return a


def _cases():
    """(entry point, the one broken argument(s), wording of the refusal)"""
    out = []
    for name in ARGS:
        bwd, q8 = "bwd" in name, name == "mic_attn_bwd_q8"
        shape_msg = "one 64x64 tile per sequence" if name in ONE_TILE else "bad shape"
        for dim in ("B", "H", "Tq", "Tk"):
            out += [(name, {dim: 0}, shape_msg), (name, {dim: -3}, shape_msg)]
        pointers = [n for n in (BWD_POINTERS if bwd else FWD_POINTERS) if n in ARGS[name].split()]
        pointers += ["q_off", "q_len"] if "packed" in name else []
        pointers += ["dq8", "dk8", "dv8"] if q8 else []
        out += [(name, {n: None}, "null pointer") for n in pointers]
        for dtype, half in ((BF16, 4), (F32, 2)):
            if not (q8 and dtype == F32):
                out += [(name, {"dtype": dtype, n: 128 + half}, "row strides must keep 16-B alignment") for n in (BWD_STRIDES if bwd else FWD_STRIDES)]
        if not q8:
            out.append((name, {"dtype": 7}, "bad dtype"))
        if name in ONE_TILE:
            out += [(name, {"Tq": 65}, "one 64x64 tile per sequence"), (name, {"Tk": 65}, "one 64x64 tile per sequence")]
        if name in TILED_PACKED:
            out += [(name, {"kv_packed": 1, "Tq": 16, "Tk": 17}, "kv_packed needs Tk == Tq_max"),
                    (name, {"kv_packed": 1, "Tq": 130, "Tk": 64}, "kv_packed needs Tk == Tq_max")]
    q8 = "mic_attn_bwd_q8"
    out += [(q8, {"dq8": _fp8_out(fmt=E4M3)}, "bad fp8 outputs"), (q8, {"dk8": _fp8_out(fmt=E4M3)}, "bad fp8 outputs"),
            (q8, {"dq8": _fp8_out(fmt=9), "dk8": _fp8_out(fmt=9)}, "bad fp8 outputs")]
    out += [(q8, {d: _fp8_out(**{f: None})}, "bad fp8 outputs") for d in ("dq8", "dk8") for f in ("q", "state")]
    out += [(q8, {"q_off": ADDR}, "null pointer"), (q8, {"q_len": ADDR}, "null pointer")]
    return out


CASES = _cases()


def test_refusal_table_covers_every_entry_point():
    assert {c[0] for c in CASES} == set(ARGS) and len(CASES) == len({repr(c) for c in CASES})


def _case_id(i):
    name, broken, _ = CASES[i]
    return "-".join([name[4:]] + [k if isinstance(v, dict) else f"{k}={v}" for k, v in broken.items()] + [str(i)])


@pytest.mark.parametrize("name,broken,wording", CASES, ids=[_case_id(i) for i in range(len(CASES))])
def test_entry_point_refuses(name, broken, wording):
    import mic_amd  # noqa: F401
    from mic_amd import _lib

    lib = _lib.lib()
    a = dict(_good(name), **broken)
    keep = []  # the descriptors stay alive over the call

    def arg(n):
        if isinstance(a[n], dict):
            keep.append(_lib.Fp8Out(**a[n]))
            return C.byref(keep[-1])
        return a[n]

    assert len(ARGS[name].split()) == len(_lib._SIGS[name][0])
    rc = getattr(lib, name)(*[arg(n) for n in ARGS[name].split()])
    msg = lib.mic_last_error().decode()
    assert rc == MIC_EINVAL, (rc, msg)
    assert msg.startswith(name + ":") and wording in msg, msg


# ---------------------------------------------------------------------------------------------------------------- engine choice
WRAPPERS = ("attn_fwd", "attn_probs", "attn_bwd", "attn_fwd_packed", "attn_bwd_packed", "attn_fwd_packed_tiled", "attn_bwd_packed_tiled",
            "attn_bwd_q8")
SHAPES = ((12, 10), (64, 64), (65, 50), (16, 65), (130, 197))


@pytest.fixture
def calls(monkeypatch):
    """the eight `ops.attn_*` wrappers replaced by recorders: [(wrapper name, its arguments by parameter name, defaults filled in)]"""
    import mic_amd  # noqa: F401
    from mic_amd import ops

    log = []
    for w in WRAPPERS:
        sig = inspect.signature(getattr(ops, w))

        def rec(*args, _w=w, _sig=sig, **kw):
            b = _sig.bind(*args, **kw)
            b.apply_defaults()
            log.append((_w, dict(b.arguments)))
        monkeypatch.setattr(ops, w, rec)
    return log


def _operands(self_attn):
    import torch

    t = {n: torch.zeros(2, 8) for n in ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "key_mask", "q_off", "q_len", "dv8")}
    ld = dict(ldq=24, ldk=24, ldv=24, ldo=8) if self_attn else dict(ldq=8, ldk=48, ldv=48, ldo=8)
    return t, ld


def _same(got, want):
    assert set(want) <= set(got), set(want) - set(got)
    for n, w in want.items():
        assert got[n] is w if (w is None or hasattr(w, "shape") or isinstance(w, SimpleNamespace)) else got[n] == w, (n, got[n], w)


@pytest.mark.parametrize("Tq,Tk", SHAPES)
@pytest.mark.parametrize("packed", (False, True))
@pytest.mark.parametrize("self_attn", (False, True))
def test_engine_forward_choice(calls, Tq, Tk, packed, self_attn):
    from mic_amd.engine import Engine

    t, ld = _operands(self_attn)
    pack = (t["q_off"], t["q_len"], 17) if packed else None
    Engine.attn_forward(SimpleNamespace(), t["q"], t["k"], t["v"], t["out"], t["lse"], 3, 2, Tq, Tk, **ld, pack=pack, kv_packed=self_attn,
                        key_mask=t["key_mask"], causal=self_attn)
    (name, got), = calls
    want = dict(q=t["q"], k=t["k"], v=t["v"], out=t["out"], lse=t["lse"], B=3, H=2, causal=self_attn, **ld)
    if packed:
        assert name == ("attn_fwd_packed_tiled" if Tq > 64 or Tk > 64 else "attn_fwd_packed")
        assert "key_mask" not in got
        want.update(Tq_max=Tq, Tk=Tk, q_off=t["q_off"], q_len=t["q_len"], kv_packed=self_attn)
    else:
        assert name == "attn_fwd"
        want.update(Tq=Tq, Tk=Tk, key_mask=t["key_mask"])
    _same(got, want)


@pytest.mark.parametrize("Tq,Tk", SHAPES)
@pytest.mark.parametrize("packed", (False, True))
@pytest.mark.parametrize("self_attn", (False, True))
@pytest.mark.parametrize("fp8", (False, True))
def test_engine_backward_choice(calls, Tq, Tk, packed, self_attn, fp8):
    from mic_amd.engine import Engine

    t, ld = _operands(self_attn)
    ld.update(lddo=8)
    pack = (t["q_off"], t["q_len"], 17) if packed else None
    dq8, dk8 = SimpleNamespace(), SimpleNamespace()  # (the `Fp8Out` descriptors: handed through as they are)
    ldg = (24, 24, 24) if self_attn else (8, 48, 48)
    grads = dict(grads8=(dq8, dk8, t["dv8"])) if fp8 else dict(grads=(t["dq"], t["dk"], t["dv"]), ldg=ldg)

    def run():
        Engine.attn_backward(SimpleNamespace(), t["q"], t["k"], t["v"], t["out"], t["dout"], t["lse"], 3, 2, Tq, Tk, **ld, **grads, pack=pack,
                             kv_packed=self_attn, key_mask=t["key_mask"], causal=self_attn)

    tiled = Tq > 64 or Tk > 64
    if fp8 and tiled:  # a caller error: fp8 targets are asked for only where the call fits one tile
        with pytest.raises(ValueError, match="one 64x64 tile"):
            run()
        assert calls == []
        return
    run()
    (name, got), = calls
    want = dict(q=t["q"], k=t["k"], v=t["v"], out=t["out"], dout=t["dout"], lse=t["lse"], B=3, H=2, causal=self_attn, **ld)
    if fp8:
        assert name == "attn_bwd_q8"
        want.update(Tq=Tq, Tk=Tk, dq8=dq8, dk8=dk8, dv8=t["dv8"], q_off=pack and t["q_off"], q_len=pack and t["q_len"],
                    kv_packed=packed and self_attn, key_mask=None if packed else t["key_mask"])
    else:
        want.update(dq=t["dq"], dk=t["dk"], dv=t["dv"], lddq=ldg[0], lddk=ldg[1], lddv=ldg[2])
        if packed:
            assert name == ("attn_bwd_packed_tiled" if tiled else "attn_bwd_packed")
            assert "key_mask" not in got
            want.update(Tq_max=Tq, Tk=Tk, q_off=t["q_off"], q_len=t["q_len"], kv_packed=self_attn)
        else:
            assert name == "attn_bwd"
            want.update(Tq=Tq, Tk=Tk, key_mask=t["key_mask"])
    _same(got, want)
