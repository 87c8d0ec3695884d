#!/usr/bin/env python3
"""Register, scratch and LDS figures of the kernels in a `--save-temps` assembly file, read from its code-object metadata.

    hipcc <the library's flags> --save-temps -c nebulae_amd/csrc/gi_query.hip -o /tmp/gi_query.o
    tools/kernel_resources.py gi_query-hip-amdgcn-amd-amdhsa-gfx950.s [name filter ...]

One line per kernel, sorted by demangled name: VGPRs, SGPRs, scratch bytes per lane (private_segment_fixed_size), LDS bytes
(group_segment_fixed_size), kernarg bytes.  Two builds compare with diff.  A developer check, not a test."""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        f = {k: v for k, v in re.findall(r"\n\s+\.(\w+):\s+(\S+)", "\n" + block)}
        if "name" in f:
            out[f["name"]] = f
    return out


def main():
    ks = kernels(sys.argv[1])
    names = sorted(ks)
    demangled = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    rows = []
    for name, nice in zip(names, demangled):
        nice = re.sub(r"\(.*", "", nice.replace("neb::(anonymous namespace)::", "").replace("void ", ""))
        if all(s in nice for s in sys.argv[2:]):
            f = ks[name]
            rows.append((nice, f["vgpr_count"], f["sgpr_count"], f["private_segment_fixed_size"], f["group_segment_fixed_size"], f["kernarg_segment_size"],
                         f["vgpr_spill_count"], f["sgpr_spill_count"]))
    print(f"{'kernel':<64} {'vgpr':>5} {'sgpr':>5} {'scratch':>8} {'lds':>6} {'kernarg':>8} {'vspill':>7} {'sspill':>7}")
    for r in sorted(rows):
        print(f"{r[0]:<64} {r[1]:>5} {r[2]:>5} {r[3]:>8} {r[4]:>6} {r[5]:>8} {r[6]:>7} {r[7]:>7}")


if __name__ == "__main__":
    main()
