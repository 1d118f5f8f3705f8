"""Per-kernel resource table of libmic_hip.so from the compiler's own listing (hipcc -Rpass-analysis=kernel-resource-usage, which the
Makefile leaves in csrc/build/<unit>.res): VGPRs / AGPRs / SGPRs, scratch, spills, occupancy (waves per SIMD), static LDS.

  python tools/kernel_resources.py            table of the current build beside the committed one, differences marked
  python tools/kernel_resources.py --update   rewrite tests/golden/kernel_resources.json from the current build (and
                                              tests/golden/kernel_resources_units.json from csrc/build/units/: the Makefile's UNIT_SRCS;
                                              tests/golden/kernel_resources_units_inc.json from csrc/build/units_inc/: INC_UNIT_SRCS;
                                              tests/golden/kernel_resources_units_tile.json from csrc/build/units_tile/: TILE_UNIT_SRCS;
                                              tests/golden/kernel_resources_units_score.json from csrc/build/units_score/: SCORE_UNIT_SRCS)

The guard (tests/test_kernel_resources_cpu.py) fails on scratch or spills in any kernel, on an occupancy below the committed one, and
on kernels the table does not know — the two silent regressions of round 4 (272 B of scratch in the non-PLAIN 256x256 epilogues, a
waterfall loop around every LDS-DMA request) both showed in exactly these numbers first."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "multilingual-image-captioning_amd", "csrc", "build")
TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources.json")
# units whose kernels are not in that table (the Makefile's UNIT_SRCS): their listings lie under build/units/, their table is this one
UNITS_BUILD = os.path.join(BUILD, "units")
UNITS_TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_units.json")
# ... and the units of that kind that include a text of the main units (the Makefile's INC_UNIT_SRCS), under build/units_inc/
INC_UNITS_BUILD = os.path.join(BUILD, "units_inc")
INC_UNITS_TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_units_inc.json")
# ... and the units of that kind built from the attention cores' tile text (TILE_UNIT_SRCS), under build/units_tile/
TILE_UNITS_BUILD = os.path.join(BUILD, "units_tile")
TILE_UNITS_TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_units_tile.json")
# ... and the units behind model.score (SCORE_UNIT_SRCS: gemm_d2_kernel<2> on gemm_d2.hip's text, the picked-logit CE and segment sums)
SCORE_UNITS_BUILD = os.path.join(BUILD, "units_score")
SCORE_UNITS_TABLE = os.path.join(ROOT, "tests", "golden", "kernel_resources_units_score.json")
FIELDS = {"TotalSGPRs": "sgpr", "VGPRs": "vgpr", "AGPRs": "agpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
          "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds"}


def parse_res(path):
    """{mangled kernel name: {field: int}} of one .res file"""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            try:
                cur[FIELDS[m.group(1)]] = int(m.group(2))
            except ValueError:
                pass
    return out


def demangle(names):
    for tool in ("c++filt", "/opt/rocm/lib/llvm/bin/llvm-cxxfilt"):
        try:
            r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, timeout=60)
            d = r.stdout.split("\n")
            if r.returncode == 0 and len(d) >= len(names):
                return dict(zip(names, d))
        except (OSError, subprocess.SubprocessError):
            pass
    return {n: n for n in names}  # (mangled names: still unique keys, the table then has to come from the same machine)


def short(name: str) -> str:
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*$", "", name)  # template arguments stay, the parameter list goes


def current(build=BUILD):
    """{unit: {kernel (demangled, short): fields}} of a build directory"""
    units = {}
    for f in sorted(os.listdir(build)) if os.path.isdir(build) else []:
        if f.endswith(".res"):
            k = parse_res(os.path.join(build, f))
            dm = demangle(list(k))
            units[f[:-4]] = {short(dm[n]): v for n, v in k.items()}
    return units


def compare(cur, ref):
    """list of (severity, message); severity "fail" = what the guard refuses"""
    msgs = []
    for unit, ks in cur.items():
        for name, v in ks.items():
            tag = f"{unit}: {name}"
            if v.get("scratch", 0) > 0 or v.get("vgpr_spill", 0) > 0:
                msgs.append(("fail", f"{tag}: scratch {v.get('scratch')} B/lane, {v.get('vgpr_spill')} VGPRs spilled"))
            r = ref.get(unit, {}).get(name)
            if r is None:
                msgs.append(("fail", f"{tag}: not in the committed table (python tools/kernel_resources.py --update)"))
                continue
            if v.get("occupancy", 0) < r.get("occupancy", 0):
                msgs.append(("fail", f"{tag}: occupancy {r['occupancy']} -> {v['occupancy']} waves/SIMD (vgpr {r.get('vgpr')}+{r.get('agpr')} -> {v.get('vgpr')}+{v.get('agpr')})"))
            if v.get("sgpr_spill", 0) > r.get("sgpr_spill", 0):  # (SGPRs spill into VGPR lanes, not memory: cheap, but a trend to see)
                msgs.append(("fail", f"{tag}: SGPR spills {r.get('sgpr_spill', 0)} -> {v['sgpr_spill']}"))
            for f in ("vgpr", "agpr", "sgpr", "lds", "occupancy"):
                if v.get(f) != r.get(f):
                    msgs.append(("note", f"{tag}: {f} {r.get(f)} -> {v.get(f)}"))
    for unit, ks in ref.items():
        for name in ks:
            if name not in cur.get(unit, {}):
                msgs.append(("note", f"{unit}: {name}: in the committed table, not in this build"))
    return msgs


def main():
    cur, cur_units, cur_inc, cur_tile = current(), current(UNITS_BUILD), current(INC_UNITS_BUILD), current(TILE_UNITS_BUILD)
    cur_score = current(SCORE_UNITS_BUILD)
    if not cur:
        sys.exit(f"no .res files under {BUILD}: build first (make -C multilingual-image-captioning_amd/csrc)")
    if "--update" in sys.argv:
        os.makedirs(os.path.dirname(TABLE), exist_ok=True)
        for table, c in ((TABLE, cur), (UNITS_TABLE, cur_units), (INC_UNITS_TABLE, cur_inc), (TILE_UNITS_TABLE, cur_tile), (SCORE_UNITS_TABLE, cur_score)):
            json.dump(c, open(table, "w"), indent=0, sort_keys=True)
            print(f"wrote {table}: {sum(len(v) for v in c.values())} kernels in {len(c)} units")
        return
    print(f"{'unit':<12} {'kernel':<88} {'vgpr':>4} {'agpr':>4} {'sgpr':>4} {'scr':>4} {'occ':>3} {'lds':>6}")
    for table, c in ((TABLE, cur), (UNITS_TABLE, cur_units), (INC_UNITS_TABLE, cur_inc), (TILE_UNITS_TABLE, cur_tile), (SCORE_UNITS_TABLE, cur_score)):
        ref = json.load(open(table)) if os.path.exists(table) else {}
        for unit, ks in c.items():
            for name, v in sorted(ks.items()):
                print(f"{unit:<12} {name[:88]:<88} {v.get('vgpr', 0):>4} {v.get('agpr', 0):>4} {v.get('sgpr', 0):>4} {v.get('scratch', 0):>4} {v.get('occupancy', 0):>3} {v.get('lds', 0):>6}")
        for sev, m in compare(c, ref):
            print(f"[{sev}] {m}")


if __name__ == "__main__":
    main()
