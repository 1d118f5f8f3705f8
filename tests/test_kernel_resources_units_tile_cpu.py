"""The regression guard of tests/test_kernel_resources_cpu.py for the units built from the attention cores' tile text (the Makefile's
TILE_UNIT_SRCS; today csrc/attention_shared.hip, the cross-attention kernels with K / V shared by G query sequences): the compiler's
per-kernel resource listing of the current build (csrc/build/units_tile/*.res) against tests/golden/kernel_resources_units_tile.json, by
the same rules (tools/kernel_resources.py compare).  No GPU needed."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "multilingual-image-captioning_amd", "csrc")


def test_shared_attention_unit_keeps_its_registers_scratch_and_occupancy():
    import kernel_resources as KR

    for f in (os.listdir(KR.TILE_UNITS_BUILD) if os.path.isdir(KR.TILE_UNITS_BUILD) else []):  # an object without its listing: make would do nothing
        if f.endswith(".o") and not os.path.exists(os.path.join(KR.TILE_UNITS_BUILD, f[:-2] + ".res")):
            os.remove(os.path.join(KR.TILE_UNITS_BUILD, f))
    subprocess.run(["make", "-C", CSRC, "-j8"], check=True, capture_output=True)  # incremental: nothing to do after build()
    cur = KR.current(KR.TILE_UNITS_BUILD)
    ref = json.load(open(KR.TILE_UNITS_TABLE))
    fails = [m for sev, m in KR.compare(cur, ref) if sev == "fail"]
    assert not fails, "\n".join(fails)
    kernels = {f"attn_{d}_shared_kernel<{t}>" for d in ("fwd", "bwd") for t in ("unsigned short", "float")}
    assert {u: set(k) for u, k in cur.items()} == {u: set(k) for u, k in ref.items()} == {"attention_shared": kernels}
    mk = open(os.path.join(CSRC, "Makefile")).read()
    units = set(re.search(r"^TILE_UNIT_SRCS\s*=\s*(.*)$", mk, re.M).group(1).replace(".hip", "").split())
    assert units == set(ref)
    # ... and none of them is in one of the other tables
    assert not units & (set(json.load(open(KR.TABLE))) | set(json.load(open(KR.UNITS_TABLE))) | set(json.load(open(KR.INC_UNITS_TABLE))))
    k = cur["attention_shared"]
    assert all(v["scratch"] == 0 and v["vgpr_spill"] == 0 and v["sgpr_spill"] == 0 and v["lds"] == 0 for v in k.values())  # (LDS is dynamic)
    # the backward holds its dK / dV blocks (2 x 16 accumulators) beside the score blocks: at least two waves per SIMD
    assert all(k[f"attn_bwd_shared_kernel<{t}>"]["occupancy"] >= 2 for t in ("unsigned short", "float"))
    # the tile text the unit shares with attention.hip is a prerequisite of both rules
    assert re.search(r"^build/units_tile/%\.o:.*\battention_tile\.h\b", mk, re.M) and re.search(r"^build/%\.o:.*\battention_tile\.h\b", mk, re.M)
