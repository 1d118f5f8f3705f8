"""mic_gemm_plan and the GEMM launcher read one dispatch decision (csrc/gemm.hip: decide).  On a machine without a GPU:
  - the decision reports what the commit before it reported: tests/golden/gemm_plan_parent.npz holds ~10 000 drawn argument sets
    (all of them pass mic_gemm's host checks) with that commit's return code and report fields, one block at the default switches
    and one per entry of util_gemm_cases.SWITCHES; every block is replayed in a child process (the switches latch) and must come
    back identical, without exception;
  - in the same children, the report follows each switch on the conformance cases that switch can change;
  - where that commit's report and that commit's LAUNCHER disagreed (the draws above stay clear of these), the launcher was the
    truth and the report now says what it did: one named test each."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import util_gemm_cases as GC  # noqa: E402

BLOCKS = ["default"] + [f"{env}={val}" for env, val, _ in GC.SWITCHES]


@pytest.fixture(scope="module")
def replays():
    """{block: the child's report}: all blocks side by side (host arithmetic only, nothing touches a GPU)"""
    base = {k: v for k, v in os.environ.items() if not k.startswith("MIC_")}
    children = []
    for block, name in enumerate(BLOCKS):
        env = dict(base, **({name.split("=")[0]: name.split("=")[1]} if block else {}))
        children.append(subprocess.Popen([sys.executable, os.path.join(HERE, "util_gemm_cases.py"), str(block)], env=env,
                                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    out = {}
    for name, ch in zip(BLOCKS, children):
        so, se = ch.communicate(timeout=600)
        assert ch.returncode == 0, (name, se[-2000:])
        out[name] = json.loads(so.strip().splitlines()[-1])
    return out


def test_fixture_is_the_sweep_it_claims():
    fx = np.load(os.path.join(HERE, GC.PLAN_FIXTURE))
    per_block = np.bincount(fx["draws"][:, 6], minlength=len(BLOCKS))
    assert per_block[0] >= 5000 and (per_block[1:] >= 300).all() and len(per_block) == len(BLOCKS)
    assert (fx["answers"][:, 0] == 0).all()
    f = {k: i + 1 for i, k in enumerate(GC.ANSWER_FIELDS)}
    a0 = fx["answers"][fx["draws"][:, 6] == 0]
    combos = np.unique(a0[:, [f[k] for k in ("tile", "tile_m", "kgroups", "blocks_per_cu", "phased")]], axis=0, return_counts=True)
    assert len(combos[0]) == 10 and combos[1].min() >= 20  # every plan the planner can produce


@pytest.mark.parametrize("block", BLOCKS)
def test_plan_reports_what_the_parent_reported(replays, block):
    r = replays[block]
    assert r["replayed"] >= 300 and r["differ"] == 0, r


@pytest.mark.parametrize("block", BLOCKS[1:])
def test_report_follows_the_switch(replays, block):
    assert replays[block]["switch_ignored"] == [], replays[block]


def _report(M, N, K, *, akm=False, bkm=False, **feats):
    return GC.plan_report(GC.case("x", M, N, K, akm=akm, bkm=bkm, **feats))


def test_clamped_split_k_launch_is_plain_and_persistent():
    """split_k = 2 on one K-tile: the launch clamps the split to 1, is PLAIN and runs as cu_budget persistent blocks.  The parent's
    report took "not PLAIN" from the unclamped split_k and answered grid = 512."""
    from mic_amd import ops

    p = ops.gemm_plan([(4096, 8192, 64)], b_kmajor=True, split_k=2, kernel=True)
    assert p["tile"] == 256 and p["blocks"] == 512 and p["plain"] == 1 and p["grid"] == p["cu_budget"] == 256
    assert GC.kernel_name(p, "bf16", False, True) == "gemm_bf16_kernel<128,64,4,64,false,true,1,true,0>"


def test_rowstat_with_n_not_a_multiple_of_128_runs_on_gemm_d2():
    """the launcher never asked for N % 128 == 0 before handing a softmax-partials launch to gemm_d2.hip (256 x 128 tiles, the last
    column tile half empty); the parent's report did and answered with the 256 x 256 tiling"""
    N = 65536 + 64
    p = _report(2404, N, 1024, bias=1, rowstat=1)
    assert GC.kernel_name(p, "bf16", False, False) == "gemm_d2_kernel<1>"
    assert (p["tile_m"], p["tile"], p["blocks_per_cu"]) == (256, 128, 2) and p["grid"] == p["blocks"] == 10 * (N // 128 + 1)


def test_rowstat_with_folded_layernorm_runs_on_gemm_w4():
    """gemm_d2.hip has no folded LayerNorm: such a launch stays on the four-wave kernel (epilogue 7); the parent's report answered
    with gemm_d2's tiling for every launch that carried rowstat"""
    p = _report(1024, 32768, 1024, ln=1, rowstat=1)
    assert GC.kernel_name(p, "bf16", False, False) == "gemm_w4_kernel<7>"
    assert (p["tile_m"], p["tile"], p["blocks_per_cu"]) == (256, 256, 1) and p["grid"] == p["blocks"] == 4 * 128


def test_rowstat_on_an_operand_of_2_gib_runs_on_the_phased_kernel():
    """the LDS-DMA kernels address an operand through a 2^31 - 1 byte buffer resource: B = [250112][4352] bf16 is larger, so the
    launch stays on the four-phase kernel (64-bit addresses, PLAIN epilogue); the parent's report answered with gemm_d2's tiling"""
    p = _report(2404, GC.V_PAD, 4352, bias=1, rowstat=1)
    assert GC.kernel_name(p, "bf16", False, False) == "gemm_phased_kernel<false,false,true>"
    assert (p["tile_m"], p["tile"], p["phased"]) == (256, 256, 2) and p["grid"] == p["blocks"] == 10 * 977
