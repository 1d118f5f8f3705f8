"""Worst err / bound per checked quantity from the `[conformance] <kernel>/<dtype> <quantity>: <case>: worst err/bound R ...` lines
two pytest -s logs print (the GPU module's, and the CPU module's numpy emulation on the same cases), side by side.
usage: python tools/conformance_worst_ratio.py <gpu log> <cpu log>"""
import re
import sys

LINE = re.compile(r"\[conformance\] (\S+/(?:bf16|f32) [^:]+): (.*): worst err/bound (\S+) over")


def worst(path):
    out = {}
    for m in LINE.finditer(open(path, errors="replace").read()):
        key, case, r = m.group(1), m.group(2), float(m.group(3))
        if r >= out.get(key, (-1.0, ""))[0]:
            out[key] = (r, case)
    return out


def main():
    gpu, cpu = worst(sys.argv[1]), worst(sys.argv[2])
    print(f"{'kernel/dtype quantity':44s} {'GPU worst':>10s}  {'at case':40s} {'emulation worst':>15s}  at case")
    for k in sorted(set(gpu) | set(cpu)):
        g, e = gpu.get(k), cpu.get(k)
        print(f"{k:44s} {g[0] if g else float('nan'):10.3g}  {(g[1] if g else '-'):40s} {e[0] if e else float('nan'):15.3g}  {e[1] if e else '-'}")


if __name__ == "__main__":
    main()
