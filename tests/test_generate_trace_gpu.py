"""The host-side launch sequence of `generate()` — every libmic_hip.so call with its scalar arguments and stream, every event
record / wait between streams — equals, call for call, the one recorded before greedy search, sampling and beam search got one
decode-chain driver (tests/golden/generate_trace_parent.json.gz, written by tests/golden/make_golden_generate_trace.py with the
modes of tests/util_generate_trace.py).  No exceptions are listed: a change that moves, adds or drops a launch or a hand-over in
one of these modes has to re-record the fixture and say why.  What the calls return: token ids and step counts equal to the
recorded ones, scores and log-likelihoods within rtol = atol = 1e-4 (the bound of tests/test_generate_gpu.py against the oracle)."""
import numpy as np
import pytest

import util_generate_trace as GT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    return GT.load_fixture()


def test_fixture_holds_every_mode(recorded):
    assert set(recorded) == set(GT.MODES) and len(GT.MODES) == 19
    for name, (lines, calls) in recorded.items():
        assert len(lines) > 100 and len(calls) == 3, name


@pytest.mark.parametrize("mode", list(GT.MODES))
def test_generate_trace_equals_the_recorded_one(dev, recorded, mode):
    want, want_calls = recorded[mode]
    got, calls = GT.run_mode(mode, dev)
    first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)
    if first is None and len(got) != len(want):
        first = min(len(got), len(want))
    assert first is None, (f"{mode}: call {first} of {len(got)} (recorded: {len(want)}) differs\n  recorded: " + " | ".join(want[max(first - 3, 0): first + 3])
                           + "\n  now:      " + " | ".join(got[max(first - 3, 0): first + 3]))
    assert len(calls) == len(want_calls)
    for i, (a, b) in enumerate(zip(calls, want_calls)):
        assert set(a) == set(b), (mode, i, sorted(a), sorted(b))
        assert a["sequences"] == b["sequences"], (mode, i)
        assert a.get("steps") == b.get("steps") and type(a.get("steps")) is type(b.get("steps")), (mode, i, a.get("steps"), b.get("steps"))
        if "scores" in b:
            x, y = np.asarray(a["scores"], dtype=np.float64), np.asarray(b["scores"], dtype=np.float64)
            print(mode, "call", i, "max |score - recorded|", float(np.abs(x - y).max()))
            assert x.shape == y.shape and np.allclose(x, y, rtol=1e-4, atol=1e-4), (mode, i, x, y)
