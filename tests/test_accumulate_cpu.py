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
