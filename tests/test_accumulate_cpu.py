"""Host logic of gradient accumulation (`Trainer(accumulate_steps=N)`), no GPU: the dropout streams of the virtual ranks and the
validation of `accumulate_steps` itself (it happens before the constructor touches the model or a device)."""
import numpy as np
import pytest


def _todays_seed(seed, rank, step):
    """the formula of `Trainer` without accumulation, restated: per-device stream (main.py:251), split per step (main.py:686)"""
    dropout_seed = (seed * 1000003 + rank * 7919) & 0xFFFFFFFF
    return (dropout_seed + step * 0x9E3779B1) & 0xFFFFFFFF


@pytest.mark.parametrize("seed,r,N,j,step", [(42, 0, 1, 0, 0), (42, 0, 2, 1, 0), (42, 1, 2, 0, 3), (7, 3, 8, 5, 1000), (0, 0, 3, 2, 1),
                                              (123456789, 7, 8, 7, 70000), (2 ** 31 - 1, 5, 4, 3, 2 ** 20)])
def test_virtual_rank_seed_is_todays_formula_at_rank_r_times_n_plus_j(seed, r, N, j, step):
    from mic_amd.train import virtual_rank_dropout_seed

    got = virtual_rank_dropout_seed(seed, r, step, N, j)
    assert got == _todays_seed(seed, r * N + j, step)
    assert 0 <= got <= 0xFFFFFFFF


def test_micro_steps_of_one_rank_draw_the_streams_of_n_ranks():
    """N micro-steps on rank 0 = the N ranks of a data-parallel run; 2 ranks x N micro-steps = 2 N distinct ranks, none drawn twice"""
    from mic_amd.train import virtual_rank_dropout_seed

    N, step = 4, 11
    assert [virtual_rank_dropout_seed(42, 0, step, N, j) for j in range(N)] == [_todays_seed(42, q, step) for q in range(N)]
    both = [virtual_rank_dropout_seed(42, r, step, N, j) for r in range(2) for j in range(N)]
    assert both == [_todays_seed(42, q, step) for q in range(2 * N)] and len(set(both)) == 2 * N
    # without accumulation the function is the Trainer's own formula
    assert virtual_rank_dropout_seed(42, 3, step) == _todays_seed(42, 3, step)


@pytest.mark.parametrize("bad", [0, -1, 2.5, True, False, "2", None, np.float32(2.0)])
def test_accumulate_steps_must_be_a_positive_integer(bad):
    from mic_amd import Trainer

    with pytest.raises(ValueError, match="accumulate_steps"):
        Trainer(None, lambda step: 1e-3, accumulate_steps=bad)


def test_accumulation_kernels_keep_their_registers_scratch_and_occupancy():
    """the guard of tests/test_kernel_resources_cpu.py for the unit this feature adds (csrc/accumulate.hip): its compiler listing
    (csrc/build/new/accumulate.res, written by `make`) against its own table — no scratch, no spilled registers, occupancy not below
    the committed one, no kernel the table does not know, none missing"""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources as KR

    subprocess.run(["make", "-C", os.path.join(root, "multilingual-image-captioning_amd", "csrc"), "-j8"], check=True, capture_output=True)
    cur = KR.current_new()
    assert "accumulate" in cur, "no listing of csrc/accumulate.hip under csrc/build/new"
    cur = {"accumulate": cur["accumulate"]}
    ref = json.load(open(KR.NEW_TABLES["accumulate"]))
    fails = [m for sev, m in KR.compare(cur, ref) if sev == "fail"]
    assert not fails, "\n".join(fails)
    assert set(cur["accumulate"]) == set(ref["accumulate"]) == {"grad_accumulate_kernel<true>", "grad_accumulate_kernel<false>",
                                                                "adamw_acc_kernel<false>", "adamw_acc_kernel<true>"}
    assert all(v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["occupancy"] == 8 for v in cur["accumulate"].values())
