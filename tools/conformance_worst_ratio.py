"""Worst err / bound per checked quantity from the `[conformance] <kernel>/<dtype> <quantity>: <case>: worst err/bound R ...` lines
two pytest -s logs print (the GPU module's, and the CPU module's numpy emulation on the same cases), side by side.
usage: python tools/conformance_worst_ratio.py <gpu log> <cpu log>
       python tools/conformance_worst_ratio.py --shares <gpu log> <cpu log>   the fp8 suite's interval-checked emitters: the largest
       share of bytes off the nominal byte ("... share off nominal S over N bytes ..."), device beside emulation"""
import re
import sys

SHARE = re.compile(r"\[conformance\] (\S+/e[45]m[32] [^:]+): (.*): share off nominal (\S+) over")
LINE = re.compile(r"\[conformance\] (\S+/(?:bf16|f32) [^:]+): (.*): worst err/bound (\S+) over")


def worst(path, line=LINE):
    out = {}
    for m in line.finditer(open(path, errors="replace").read()):
        key, case, r = m.group(1), m.group(2), float(m.group(3))
        if r >= out.get(key, (-1.0, ""))[0]:
            out[key] = (r, case)
    return out


def main():
    if sys.argv[1] == "--shares":
        gpu, cpu = worst(sys.argv[2], SHARE), worst(sys.argv[3], SHARE)
        what = "emitter/format tensor"
    else:
        gpu, cpu = worst(sys.argv[1]), worst(sys.argv[2])
        what = "kernel/dtype quantity"
    print(f"{what:44s} {'GPU worst':>10s}  {'at case':40s} {'emulation worst':>15s}  at case")
    for k in sorted(set(gpu) | set(cpu)):
        g, e = gpu.get(k), cpu.get(k)
        print(f"{k:44s} {g[0] if g else float('nan'):10.3g}  {(g[1] if g else '-'):40s} {e[0] if e else float('nan'):15.3g}  {e[1] if e else '-'}")


if __name__ == "__main__":
    main()
