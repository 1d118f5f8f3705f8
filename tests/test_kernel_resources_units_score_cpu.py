"""The regression guard of tests/test_kernel_resources_cpu.py for the units behind model.score (the Makefile's SCORE_UNIT_SRCS:
csrc/gemm_d2_pick.hip, the third epilogue instantiation of gemm_d2.hip's kernel — softmax partials and picked values, no logits —, and
csrc/score_rows.hip, the picked-logit cross-entropy and the segment sums): the compiler's per-kernel resource listing of the current
build (csrc/build/units_score/*.res) against tests/golden/kernel_resources_units_score.json, by the same rules
(tools/kernel_resources.py compare).  And that the main units the two share a text with keep exactly the kernels of their own table: the
new instantiation did not land in gemm_d2.hip's object.  No GPU needed."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "multilingual-image-captioning_amd", "csrc")


def test_score_units_keep_their_registers_scratch_and_occupancy():
    import kernel_resources as KR

    for f in (os.listdir(KR.SCORE_UNITS_BUILD) if os.path.isdir(KR.SCORE_UNITS_BUILD) else []):  # an object without its listing: make would do nothing
        if f.endswith(".o") and not os.path.exists(os.path.join(KR.SCORE_UNITS_BUILD, f[:-2] + ".res")):
            os.remove(os.path.join(KR.SCORE_UNITS_BUILD, f))
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)  # incremental: nothing to do after build()
    cur = KR.current(KR.SCORE_UNITS_BUILD)
    ref = json.load(open(KR.SCORE_UNITS_TABLE))
    fails = [m for sev, m in KR.compare(cur, ref) if sev == "fail"]
    assert not fails, "\n".join(fails)
    want = {"gemm_d2_pick": {"gemm_d2_kernel<2>"}, "score_rows": {"picked_nll_rows_kernel", "segment_sums_kernel"}}
    assert {u: set(k) for u, k in cur.items()} == {u: set(k) for u, k in ref.items()} == want
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = set(re.search(r"^SCORE_UNIT_SRCS\s*=\s*(.*)$", mk, re.M).group(1).replace(".hip", "").split())
    assert units == set(ref)
    # ... and none of them is in one of the other tables
    others = [json.load(open(t)) for t in (KR.TABLE, KR.UNITS_TABLE, KR.INC_UNITS_TABLE, KR.TILE_UNITS_TABLE)]
    assert not units & set().union(*others)
    assert all(v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0 for k in cur.values() for v in k.values())
    # the head kernel without logits: two blocks per CU like <0> and <1>, and no more registers than the instantiation that stores them
    main = KR.current()
    d2 = cur["gemm_d2_pick"]["gemm_d2_kernel<2>"]
    assert d2["occupancy"] == 2 and d2["agpr"] == 0 and d2["vgpr"] <= main["gemm_d2"]["gemm_d2_kernel<1>"]["vgpr"]
    assert cur["score_rows"]["picked_nll_rows_kernel"]["occupancy"] == 8 and cur["score_rows"]["segment_sums_kernel"]["occupancy"] == 8
    # the main units whose text these units include hold exactly the kernels their own table knows
    table = json.load(open(KR.TABLE))
    assert set(main["gemm_d2"]) == set(table["gemm_d2"]) == {"gemm_d2_kernel<0>", "gemm_d2_kernel<1>"}
    assert set(main["elementwise"]) == set(table["elementwise"])
    # the shared texts are prerequisites of both rules
    assert re.search(r"^build/units_score/%\.o:.*\bgemm_d2\.hip\b.*\bce_tiles_merge\.h\b", mk, re.M)
    assert re.search(r"^build/%\.o:.*\bce_tiles_merge\.h\b", mk, re.M)
