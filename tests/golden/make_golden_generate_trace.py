"""Writes tests/golden/generate_trace_parent.json.gz: the launch sequence (tests/util_generate_trace.py) of three `generate()`
calls in each of util_generate_trace.MODES, with the token ids, scores and step counts those calls returned, recorded on the commit
BEFORE greedy search, sampling and beam search got one decode-chain driver (run it on a checkout of that commit, with this file
and tests/util_generate_trace.py copied in and the library built, on an MI355X; it is kept for the record, the fixture is not
meant to be regenerated on later commits).  tests/test_generate_trace_gpu.py replays the modes on the current code and asks for
the identical sequence, identical ids and step counts, and scores within 1e-4.

Determinism: the whole set of modes is recorded twice, in two fresh processes, and the two records must agree line for line, in
every token id and step count, and in the scores to 1e-4 (the first record's are stored).  What the recorder leaves out by
construction is listed in tests/golden/make_golden_step_trace.py."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import util_generate_trace as GT  # noqa: E402


def record(path):
    import torch

    dev = torch.device("cuda:0")
    runs = {}
    for name in GT.MODES:
        runs[name] = GT.run_mode(name, dev)
        print(f"recorded {name}: {len(runs[name][0])} calls", flush=True)
    with open(path, "w") as f:
        json.dump(GT.pack(runs), f)


def _close(a, b) -> bool:
    import numpy as np

    return np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=1e-4, atol=1e-4)


def main():
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIC_")}
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i in range(2):
            path = os.path.join(tmp, f"rec{i}.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--record", path], env=env, check=True)
            with open(path) as f:
                recs.append(json.load(f))
    a, b = recs
    assert a["lines"] == b["lines"], "the two records differ in their lines"
    for name in GT.MODES:
        ma, mb = a["modes"][name], b["modes"][name]
        assert ma["seq"] == mb["seq"], f"{name}: the two records differ in their sequence"
        assert len(ma["calls"]) == len(mb["calls"]) == 3
        for ca, cb in zip(ma["calls"], mb["calls"]):
            assert ca["sequences"] == cb["sequences"] and ca.get("steps") == cb.get("steps"), (name, ca, cb)
            assert ("scores" in ca) == ("scores" in cb) and ("scores" not in ca or _close(ca["scores"], cb["scores"])), (name, ca, cb)
    with gzip.GzipFile(GT.FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(a, separators=(",", ":")).encode())
    print(f"{GT.FIXTURE}: {len(a['lines'])} distinct lines, {os.path.getsize(GT.FIXTURE)} bytes")
    for name in GT.MODES:
        m = a["modes"][name]
        per_step = sum(1 for i in m["seq"] if a["lines"][i].startswith(("mic_greedy_step(", "mic_beam_step(", "mic_beam_step_groups(")))
        print(f"  {name}: {len(m['seq'])} calls, {per_step} step launches, steps {[c.get('steps') for c in m['calls']]}, "
              f"first ids {[c['sequences'][0][:6] if isinstance(c['sequences'][0][0], int) else c['sequences'][0][0][:6] for c in m['calls']]}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        record(sys.argv[2])
    else:
        main()
