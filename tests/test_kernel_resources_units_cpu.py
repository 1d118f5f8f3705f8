"""The regression guard of tests/test_kernel_resources_cpu.py for the units whose kernels are not in its table (the Makefile's UNIT_SRCS;
today csrc/sample_keyed.hip): the compiler's per-kernel resource listing of the current build (csrc/build/units/*.res) against
tests/golden/kernel_resources_units.json, by the same rules (tools/kernel_resources.py compare) — no scratch, no spilled VGPRs, no
occupancy below the committed one, no more spilled SGPRs, no kernel the table does not know — and no unit or kernel of the table missing
from the build.  No GPU needed."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "multilingual-image-captioning_amd", "csrc")


def test_added_units_keep_their_registers_scratch_and_occupancy():
    import kernel_resources as KR

    for f in (os.listdir(KR.UNITS_BUILD) if os.path.isdir(KR.UNITS_BUILD) else []):  # an object without its listing: make would do nothing
        if f.endswith(".o") and not os.path.exists(os.path.join(KR.UNITS_BUILD, f[:-2] + ".res")):
            os.remove(os.path.join(KR.UNITS_BUILD, f))
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)  # incremental: nothing to do after build()
    cur = KR.current(KR.UNITS_BUILD)
    ref = json.load(open(KR.UNITS_TABLE))
    fails = [m for sev, m in KR.compare(cur, ref) if sev == "fail"]
    assert not fails, "\n".join(fails)
    assert {u: set(k) for u, k in cur.items()} == {u: set(k) for u, k in ref.items()}  # nothing of the table missing from the build
    # the units the Makefile names are the units of the table, and none of them is also in the main table
    units = set(re.search(r"^UNIT_SRCS\s*=\s*(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).replace(".hip", "").split())
    assert units == set(ref) and not units & set(json.load(open(KR.TABLE)))
    assert all(v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 for k in cur.values() for v in k.values())


def test_sampling_kernel_fits_a_1024_thread_block():
    """sample_rows_keyed_kernel runs 1024 threads per block: 16 waves on a CU's 4 SIMDs, so at most 128 VGPRs; both instantiations, the
    forced-token fill beside them, 8 waves per SIMD"""
    import kernel_resources as KR

    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)
    k = KR.current(KR.UNITS_BUILD)["sample_keyed"]
    assert set(k) == {"sample_rows_keyed_kernel<float>", "sample_rows_keyed_kernel<unsigned short>", "keyed_fill_i32_kernel"}
    for name, v in k.items():
        assert v["vgpr"] + v["agpr"] <= 128 and v["occupancy"] == 8 and v["scratch"] == 0, (name, v)
