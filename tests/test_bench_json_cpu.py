"""bench.py reads the committed PMC summaries (profiles/r*_pmc_hbm_traffic.json) for `roofline.traffic`: every such file must carry
the keys it reads (a missing key there would end the driver's bench run with a KeyError after the timed steps)."""
import glob
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_committed_pmc_summaries_carry_the_keys_bench_reads():
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json")))
    assert files
    for f in files:
        d = json.load(open(f))
        name = os.path.basename(f)
        if "generate" in name:
            att = d.get("attention", d)
            assert att["bytes_per_launch"] > 0, name
            if "gemm" in d:
                assert d["gemm"]["bytes_per_launch"] > 0, name
        else:
            assert d["bytes_per_launch"] > 0, name
        assert isinstance(d.get("summary", ""), str) and isinstance(d.get("commit", ""), str)


def test_bench_parses_and_defaults_to_one_gpu():
    import ast

    src = open(os.path.join(ROOT, "bench.py")).read()
    ast.parse(src)
    assert 'ap.add_argument("--gpus", type=int, default=1)' in src and '"--steps", type=int, default=10' in src


def test_plain_run_leaves_the_side_legs_to_full():
    """`bench.py --gpus 1 --steps N --warmup W` times the headline only; every leg beside it runs with --full"""
    import bench

    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    assert a.no_cpu_baseline and a.no_roofline and a.no_generate and a.no_dense_leg and a.no_fp8_leg and a.no_extra_legs
    assert a.emulate_comm == ""
    f = bench.parse_args(["--gpus", "1", "--full", "--dump-outputs", "out"])
    assert not (f.no_cpu_baseline or f.no_roofline or f.no_generate or f.no_dense_leg or f.no_fp8_leg or f.no_extra_legs)
    assert f.emulate_comm is None and f.dump_outputs == "out"
