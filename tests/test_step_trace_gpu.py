"""The host-side launch sequence of Trainer steps — every libmic_hip.so call with its scalar arguments and stream, every event
record / wait between streams — equals, call for call, the one recorded before the fp8 operand state moved into fp8_state.py and the
train step got one body (tests/golden/step_trace_parent.json.gz, written by tests/golden/make_golden_step_trace.py with the
recorder of tests/util_step_trace.py).  No exceptions are listed: a change that moves, adds or drops a launch or a hand-over in one
of these modes has to re-record the fixture and say why.  Losses: within 2e-4 relative of the recorded ones (same bytes, another
order of fp32 atomics — the bound of tests/test_fp8_gpu.py for that)."""
import pytest

import util_step_trace as ST

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return ST.load_fixture()


def test_fixture_holds_every_mode(recorded):
    assert set(recorded) == set(ST.MODES)
    for name, (lines, losses) in recorded.items():
        assert len(lines) > 500 and len(losses) == ST.TRAIN_STEPS + 1, name


@pytest.mark.parametrize("mode", list(ST.MODES))
def test_step_trace_equals_the_recorded_one(dev, recorded, mode):
    want, want_losses = recorded[mode]
    got, losses = ST.run_mode(mode, dev)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
    if first is None and len(got) != len(want):
        first = min(len(got), len(want))
    assert first is None, (f"{mode}: call {first} of {len(got)} (recorded: {len(want)}) differs\n  recorded: " + " | ".join(want[max(first - 3, 0): first + 3])
                           + "\n  now:      " + " | ".join(got[max(first - 3, 0): first + 3]))
    print(mode, "losses", losses, "recorded", want_losses)
    for a, b in zip(losses, want_losses):
        assert abs(a - b) <= 2e-4 * abs(b), (mode, losses, want_losses)
