"""Host logic of gradient clipping (`Trainer(max_grad_norm=c)`), no GPU: the validation of `max_grad_norm` (it happens before the
constructor touches the model or a device) and the launch geometry of the sum of squares."""
import math

import numpy as np
import pytest


@pytest.mark.parametrize("bad", [True, False, float("nan"), np.float32("nan"), 0, 0.0, -1, -0.5, -math.inf, "1.0", "inf", [1.0], 1 + 0j])
def test_max_grad_norm_must_be_none_or_a_positive_real(bad):
    from mic_amd import Trainer

    with pytest.raises(ValueError, match="max_grad_norm"):
        Trainer(None, lambda step: 1e-3, max_grad_norm=bad)


def test_max_grad_norm_is_validated_behind_accumulate_steps_and_in_front_of_the_model():
    """a bad accumulate_steps is reported first (the order of the keywords), and emulate_comm is refused with the option's name before
    the (absent) model is looked at"""
    from mic_amd import Trainer

    with pytest.raises(ValueError, match="accumulate_steps"):
        Trainer(None, lambda step: 1e-3, accumulate_steps=0, max_grad_norm=-1.0)
    for ok in (1.0, 1, np.float32(0.5), math.inf):
        with pytest.raises(ValueError, match="max_grad_norm.*emulate_comm"):
            Trainer(None, lambda step: 1e-3, max_grad_norm=ok, emulate_comm=8)


def test_grad_sumsq_slots_is_the_launch_geometry():
    """one slot per block of 256 threads x one float4, capped at 1024 blocks; host arithmetic of the library (no device)"""
    from mic_amd import ops

    assert [ops.grad_sumsq_slots(n) for n in (0, 4, 1024, 1028, 4100)] == [0, 1, 1, 2, 5]
    cap = ops.grad_sumsq_slots(1 << 40)
    assert cap == 1024
    assert ops.grad_sumsq_slots(cap * 1024) == cap and ops.grad_sumsq_slots(cap * 1024 - 4) == cap and ops.grad_sumsq_slots((cap - 1) * 1024) == cap - 1
    assert ops.grad_sumsq_slots(cap * 1024 + 4 * 1031) == cap
