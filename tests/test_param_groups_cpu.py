"""Trainer(param_groups=...) on the host: the merged-run table (`param_group_table`) over the reduced config's layout, the ready-made
matchers, every refusal, and the resource guard of the grouped AdamW's translation unit.  No GPU needed."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "multilingual-image-captioning_amd", "csrc")


def small_store():
    from mic_amd.params import ParamStore
    from util_small import product_config, ref_config

    return ParamStore(product_config(ref_config()), torch.float32, "cpu", allocate=False)


def seg_of(st, x):
    """name of the segment whose range (its alignment padding included) holds flat offset x"""
    segs = sorted(st.segs.values(), key=lambda s: s.offset)
    return [s for s in segs if s.offset <= x][-1].name


def check_cover(st, runs):
    assert runs[0][0] == 0 and runs[-1][1] == st.numel
    for (b, e, lr_scale, wd, frozen) in runs:
        assert b < e and b % 64 == 0 and e % 64 == 0
        assert isinstance(frozen, bool) and isinstance(lr_scale, float) and isinstance(wd, float)
    for a, b in zip(runs, runs[1:]):
        assert a[1] == b[0]            # sorted, gap-free
        assert a[2:] != b[2:]          # adjacent equal runs are merged


def test_table_covers_the_buffer_sorted_gap_free_and_aligned():
    from mic_amd.train import ENCODER, NO_DECAY, param_group_table

    st = small_store()
    assert st.master is None  # layout only
    for groups in ([dict(match=".*")], [dict(match=NO_DECAY, weight_decay=0.0)], [dict(match=ENCODER, frozen=True)],
                   [dict(match=r"dec\d+\..*\.w", lr_scale=0.5), dict(match=ENCODER, frozen=True), dict(match=NO_DECAY, weight_decay=0.0)],
                   [dict(match=lambda n: n.endswith(".g"), lr_scale=2.0)]):
        check_cover(st, param_group_table(st, groups, 0.01))
    # one catch-all group: one run with its settings; an empty list: one run with the Trainer's
    assert param_group_table(st, [dict(match=".*", lr_scale=0.25, weight_decay=0.5)], 0.01) == [(0, st.numel, 0.25, 0.5, False)]
    assert param_group_table(st, [], 0.01) == [(0, st.numel, 1.0, 0.01, False)]
    # alignment padding goes with the segment in front of it: vit.cls (128 elements) is the last segment, the buffer ends at a multiple of 256
    last = sorted(st.segs.values(), key=lambda s: s.offset)[-1]
    runs = param_group_table(st, [dict(match=re.escape(last.name), lr_scale=3.0)], 0.0)
    assert runs[-1] == (last.offset, st.numel, 3.0, 0.0, False) and st.numel >= last.offset + last.numel
    flb = st.segs["flb"]  # 1003 -> Vpad 1024 elements, padded to the next segment's offset
    runs = param_group_table(st, [dict(match="flb", weight_decay=0.0)], 0.01)
    assert runs[0] == (0, st.segs["shared"].offset, 1.0, 0.0, False) and runs[0][1] >= flb.numel


def test_encoder_and_no_decay_give_a_handful_of_runs():
    """flat order: flb | shared, decoder weights, vp.w | ViT weights, patch.w || decoder biases, vp.b | ViT biases | decoder LayerNorms |
    dec.pos | ViT LayerNorms, vit.pos, vit.cls"""
    from mic_amd.train import ENCODER, NO_DECAY, param_group_table

    st = small_store()
    wd = 0.01
    runs = param_group_table(st, [dict(match=ENCODER, frozen=True), dict(match=NO_DECAY, weight_decay=0.0)], wd)
    check_cover(st, runs)
    nd, dec, fr = (1.0, 0.0, False), (1.0, wd, False), (0.0, 0.0, True)
    assert [r[2:] for r in runs] == [nd, dec, fr, nd, fr, nd, dec, fr]
    firsts = [seg_of(st, r[0]) for r in runs]
    assert firsts == ["flb", "shared", f"vit{st.vL - 1}.fc2.w", f"dec{st.L - 1}.fc2.b", f"vit{st.vL - 1}.fc2.b", "dec.ln_f.g", "dec.pos", "vit0.ln1.g"]
    assert seg_of(st, runs[2][1] - 1) == "patch.w" and runs[2][1] == st.atomic_begin and seg_of(st, runs[3][1] - 1) == "vp.b"
    # the matchers themselves
    enc = {n for n in st.segs if re.fullmatch(ENCODER, n)}
    assert enc == {n for n in st.segs if n.startswith("vit") or n == "patch.w"} and "vp.w" not in enc and "vp.b" not in enc
    ndc = {n for n in st.segs if re.fullmatch(NO_DECAY, n)}
    assert ndc == {n for n in st.segs if n.endswith(".b") or n.endswith(".g") or n == "flb"}
    assert not ndc & {"shared", "dec.pos", "vit.pos", "vit.cls"} and {"dec0.ln_sa.g", "vit1.qkv.b", "vp.b", "flb"} <= ndc


def test_first_match_wins_and_unmatched_segments_keep_the_trainers_settings():
    from mic_amd.train import NO_DECAY, param_group_table

    st = small_store()
    a = param_group_table(st, [dict(match=r"dec0\.qkv\.b", lr_scale=7.0), dict(match=NO_DECAY, weight_decay=0.0)], 0.3)
    b = param_group_table(st, [dict(match=NO_DECAY, weight_decay=0.0), dict(match=r"dec0\.qkv\.b", lr_scale=7.0)], 0.3)
    s = st.segs["dec0.qkv.b"]
    at = lambda runs, x: [r for r in runs if r[0] <= x < r[1]][0][2:]
    assert at(a, s.offset) == (7.0, 0.3, False)      # its own group first: the Trainer's weight decay, not NO_DECAY's
    assert at(b, s.offset) == (1.0, 0.0, False)      # NO_DECAY first: the later group never applies
    assert at(a, st.segs["shared"].offset) == at(b, st.segs["shared"].offset) == (1.0, 0.3, False)
    # a list of regexes and a callable
    c = param_group_table(st, [dict(match=["vp\\.w", "shared"], lr_scale=0.5), dict(match=lambda n: n == "vp.b", frozen=True)], 0.0)
    assert at(c, st.segs["vp.w"].offset) == at(c, st.segs["shared"].offset) == (0.5, 0.0, False)
    assert at(c, st.segs["vp.b"].offset) == (0.0, 0.0, True)
    # regexes are applied with fullmatch: "vit" alone names nothing
    with pytest.raises(ValueError, match="matches no parameter segment"):
        param_group_table(st, [dict(match="vit")], 0.0)


BAD = [
    ("not a list", dict(match=".*")),
    ("not a list", ({"match": ".*"},)),
    ("list of dicts", [("match", ".*")]),
    ("unknown key", [dict(match=".*", lr=0.1)]),
    ("missing", [dict(lr_scale=1.0)]),
    ("match", [dict(match=5)]),
    ("match", [dict(match=[])]),
    ("matches no", [dict(match="nothing_like_this")]),
    ("matches no", [dict(match=".*"), dict(match=lambda n: False)]),
    ("lr_scale", [dict(match=".*", lr_scale=-0.5)]),
    ("lr_scale", [dict(match=".*", lr_scale=math.inf)]),
    ("lr_scale", [dict(match=".*", lr_scale=math.nan)]),
    ("lr_scale", [dict(match=".*", lr_scale="1")]),
    ("lr_scale", [dict(match=".*", lr_scale=True)]),
    ("weight_decay", [dict(match=".*", weight_decay=math.inf)]),
    ("weight_decay", [dict(match=".*", weight_decay=math.nan)]),
    ("weight_decay", [dict(match=".*", weight_decay=None)]),
    ("frozen", [dict(match=".*", frozen=1)]),
    ("frozen", [dict(match=".*", frozen="yes")]),
]


@pytest.mark.parametrize("i", range(len(BAD)))
def test_malformed_groups_raise_value_error(i):
    from mic_amd import Trainer
    from mic_amd.train import param_group_table

    _, groups = BAD[i]
    st = small_store()
    with pytest.raises(ValueError):
        param_group_table(st, groups, 0.0)

    class Model:  # a store's layout and nothing else: the Trainer must refuse before it allocates or launches anything
        store, engine = st, object()

    with pytest.raises(ValueError):
        Trainer(Model(), lambda s: 1e-3, param_groups=groups)
    assert st.grad is None and st.m is None
    # negative weight decay and lr_scale = 0 are legal
    assert param_group_table(st, [dict(match=".*", weight_decay=-0.1, lr_scale=0, frozen=np.bool_(False))], 0.0) == [(0, st.numel, 0.0, -0.1, False)]


@pytest.mark.parametrize("kw,word", [(dict(gemm_dtype="fp8"), "gemm_dtype='fp8'"), (dict(accumulate_steps=2), "accumulate_steps"),
                                     (dict(max_grad_norm=1.0), "max_grad_norm"), (dict(emulate_comm=8), "emulate_comm")])
def test_refused_combinations_fail_before_the_model_is_touched(kw, word):
    from mic_amd import Trainer

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name}) before the refusal")

    with pytest.raises(ValueError, match=f"param_groups is not supported together with {word}"):
        Trainer(Untouchable(), lambda s: 1e-3, param_groups=[dict(match=".*")], **kw)


def test_grouped_adamw_unit_keeps_its_registers_scratch_and_occupancy():
    """tools/kernel_resources.py compare on csrc/build/units_inc/ (the Makefile's INC_UNIT_SRCS) against
    tests/golden/kernel_resources_units_inc.json: no scratch, no spills, no kernel the table does not know, none missing"""
    import kernel_resources as KR

    for f in (os.listdir(KR.INC_UNITS_BUILD) if os.path.isdir(KR.INC_UNITS_BUILD) else []):  # an object without its listing: make would do nothing
        if f.endswith(".o") and not os.path.exists(os.path.join(KR.INC_UNITS_BUILD, f[:-2] + ".res")):
            os.remove(os.path.join(KR.INC_UNITS_BUILD, f))
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)  # incremental: nothing to do after build()
    cur = KR.current(KR.INC_UNITS_BUILD)
    ref = json.load(open(KR.INC_UNITS_TABLE))
    fails = [m for sev, m in KR.compare(cur, ref) if sev == "fail"]
    assert not fails, "\n".join(fails)
    assert {u: set(k) for u, k in cur.items()} == {u: set(k) for u, k in ref.items()} == {"optimizer_groups": {"adamw_groups_kernel"}}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = set(re.search(r"^INC_UNIT_SRCS\s*=\s*(.*)$", mk, re.M).group(1).replace(".hip", "").split())
    assert units == set(ref)
    # ... and none of them is in one of the other two tables or lists
    assert not units & (set(json.load(open(KR.TABLE))) | set(json.load(open(KR.UNITS_TABLE))))
    assert all(v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 for k in cur.values() for v in k.values())
    # the include the unit shares with optimizer.hip is a prerequisite of its rule
    assert re.search(r"^build/units_inc/%\.o:.*\badamw_update\.inc\b", mk, re.M)
