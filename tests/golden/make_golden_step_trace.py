"""Writes tests/golden/step_trace_parent.json.gz: the launch sequence (tests/util_step_trace.py) of 4 `train_step` calls and one
`eval_step` in each of util_step_trace.MODES, with the losses those calls returned, recorded on the commit BEFORE the fp8 operand
state moved into fp8_state.py and the two bodies of the train step became one (run it on a checkout of that commit, with this file
and tests/util_step_trace.py copied in and the library built, on an MI355X; it is kept for the record, the fixture is not meant to
be regenerated on later commits).  tests/test_step_trace_gpu.py replays the modes on the current code and asks for the identical
sequence and for losses within 2e-4 relative.

Determinism: the whole set of modes is recorded twice, in two fresh processes, and the two records must agree line for line
(the losses may differ in the order of fp32 atomics and are compared at 2e-4 relative; the first record's are stored).  They did, on
every field the recorder keeps, so nothing it keeps had to be dropped.  What the recorder leaves out by construction: pointer values
(kept as null / non-null; buffer identity was not added), stream handles and event addresses (numbered by first appearance
instead) and the creation of the process-wide CU-masked streams (`mic_stream_create_cu_masked`: issued once per process by
whoever asks first, so it belongs to the process's history, not to a step)."""
import gzip
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import util_step_trace as ST  # noqa: E402


def record(path):
    import torch

    dev = torch.device("cuda:0")
    runs = {name: ST.run_mode(name, dev) for name in ST.MODES}
    with open(path, "w") as f:
        json.dump(ST.pack(runs), f)


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
    for name in ST.MODES:
        ma, mb = a["modes"][name], b["modes"][name]
        assert ma["seq"] == mb["seq"], f"{name}: the two records differ in their sequence"
        assert len(ma["losses"]) == ST.TRAIN_STEPS + 1
        assert all(abs(x - y) <= 2e-4 * abs(x) for x, y in zip(ma["losses"], mb["losses"])), (name, ma["losses"], mb["losses"])
    with gzip.GzipFile(ST.FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(a, separators=(",", ":")).encode())
    print(f"{ST.FIXTURE}: {len(a['lines'])} distinct lines, {os.path.getsize(ST.FIXTURE)} bytes")
    for name in ST.MODES:
        print(f"  {name}: {len(a['modes'][name]['seq'])} calls, losses {a['modes'][name]['losses']} / {b['modes'][name]['losses']}")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        record(sys.argv[2])
    else:
        main()
