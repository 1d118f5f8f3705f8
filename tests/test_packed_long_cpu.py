"""Packed decoder rows beyond one attention tile, the parts that need no GPU: the two entry points are declared, bound and wrapped,
the header states their contract, the engine's choice between the one-tile and the tiled packed cores over a table of (T, S), the
case table's shapes, and the valid-row share of a seq-128 benchmark batch."""
import inspect
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NEW = ("mic_attn_fwd_packed_tiled", "mic_attn_bwd_packed_tiled")


def test_packed_tiled_entry_points_are_declared_bound_and_wrapped():
    import mic_amd  # noqa: F401
    from mic_amd import _lib, ops

    hdr = open(os.path.join(ROOT, "include", "mic_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS
        assert re.search(rf"^int\s+{name}\s*\(", hdr, flags=re.M), f"{name} is not declared in include/mic_hip.h"
        assert hasattr(_lib.lib(), name)
        one_tile = name.replace("_tiled", "")
        assert _lib._SIGS[name] == _lib._SIGS[one_tile], f"{name}: the argument list of {one_tile}"
        wrapper, wrapper1 = getattr(ops, name[4:]), getattr(ops, one_tile[4:])
        assert inspect.signature(wrapper) == inspect.signature(wrapper1)
    # the contract stands beside the declarations: the lse layout and what is never written
    doc = hdr[hdr.index("Packed rows of any length"): hdr.index("int mic_attn_fwd_packed_tiled")]
    assert "lse[(b*H + h)*Tq_max + i]" in doc and "Nothing behind q_len[b] is written" in doc


def _mirror(T, S):
    """(self-attention tiled, cross-attention tiled): the one-tile packed cores while queries and keys fit one 64x64 tile"""
    return T > 64, (T > 64 or S > 64)


def test_engine_picks_the_tiled_packed_cores_beyond_one_tile():
    from mic_amd.engine import packed_attn_tiled

    table = {(1, 1): (False, False), (12, 10): (False, False), (64, 50): (False, False), (64, 64): (False, False),
             (65, 50): (True, True), (72, 10): (True, True), (128, 50): (True, True), (130, 197): (True, True),
             (16, 65): (False, True), (64, 197): (False, True), (64, 65): (False, True), (1024, 50): (True, True)}
    for (T, S), want in table.items():
        assert _mirror(T, S) == want
        assert (packed_attn_tiled(T, T), packed_attn_tiled(T, S)) == want, (T, S)


def test_check_pack_keeps_bf16_storage_and_drops_the_lengths():
    """Engine._check_pack on a stand-in for the engine (it reads the storage type only): any T and any number of encoder positions
    pass in bfloat16 storage, fp32 storage is refused, and the row count must still be the compacted head's"""
    from types import SimpleNamespace

    import pytest
    import torch

    from mic_amd.engine import Engine

    pack, rows = ("q_off", "q_len", 300), ("idx", 300)
    for T, S in ((12, 10), (64, 50), (72, 10), (128, 50), (16, 65), (130, 197), (1024, 577)):
        eng = SimpleNamespace(dt=torch.bfloat16, P=SimpleNamespace(S=S))
        assert Engine._check_pack(eng, pack, rows, T) is pack
        assert Engine._check_pack(eng, None, rows, T) is None
        with pytest.raises(ValueError, match="compacted LM head"):
            Engine._check_pack(eng, pack, ("idx", 299), T)
        with pytest.raises(ValueError, match="bfloat16"):
            Engine._check_pack(SimpleNamespace(dt=torch.float32, P=SimpleNamespace(S=S)), pack, rows, T)


def test_case_table_holds_the_block_edges():
    import util_attn_packed_tiled_cases as PC

    got = {(c["Tq_max"], c["Tk"], tuple(c["q_len"]), c["kv_packed"]) for c in PC.SELF + PC.CROSS}
    want = {(65, 65, (1, 64, 65, 33), 1), (128, 128, (128, 1, 64, 65, 127, 128, 9), 1), (130, 130, (130, 129, 3, 64), 1),
            (200, 200, (200, 1, 137, 64, 192), 1), (48, 48, (48, 1, 33), 1),
            (128, 50, (128, 1, 65, 64, 40), 0), (65, 64, (65, 1, 64), 0), (64, 197, (64, 1, 33), 0), (130, 197, (130, 65, 7), 0)}
    assert got == want
    assert all(c["causal"] == bool(c["kv_packed"]) and c["layout"] == ("fused3" if c["kv_packed"] else "kv2") and 2 <= c["H"] <= 3
               for c in PC.SELF + PC.CROSS)
    assert {(c["Tq_max"], c["Tk"], c["kv_packed"]) for c in PC.TWINS} == {(128, 128, 1), (130, 130, 1), (128, 50, 0)}
    assert all(set(c["q_len"]) == {c["Tq_max"]} for c in PC.TWINS)
    for kind, Tk in (("self", 128), ("cross", 50)):
        c = PC.product_case(kind)
        assert (c["B"], c["H"], c["Tq_max"], c["Tk"]) == (64, 16, 128, Tk) and min(c["q_len"]) >= 10 and max(c["q_len"]) <= 128


def test_valid_row_share_of_a_seq128_benchmark_batch():
    """n ~ U{8..126} tokens + language code + eos: E[rows] / 128 = (67 + 2) / 128 = 0.539; the sample mean over 20 batches of 64
    (std of one length 34.4, of the share of 1280 lengths 0.0075) stays within five of those"""
    import bench

    share = np.mean([bench.synth_batch(64, 128, 1000, 1, seed=s)["attention_mask"].mean() for s in range(20)])
    assert abs(share - 69 / 128) < 5 * 0.0075, share
