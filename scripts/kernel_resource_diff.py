"""Compile-time resource usage of every kernel, two trees compared.

    python scripts/kernel_resource_diff.py PARENT_TREE [THIS_TREE] [--show REGEX]

Cross-compiles every .hip source of pyharp_amd/csrc of both trees with
`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` (per-source extra
flags as pyharp_amd/_build.py's EXTRA; no GPU needed) and compares TotalSGPRs, VGPRs,
AGPRs, scratch, occupancy, spills and LDS size of every kernel symbol the parent has, by
mangled name: a change that must leave existing kernels alone prints 0 differences.
--show lists the figures of THIS_TREE's kernels whose demangled name matches REGEX.
profiles/flx/resource_usage_diff.txt is this script's output for hd_solve_flx.
"""

import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pyharp_amd import _build  # noqa: E402

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", r"ScratchSize \[bytes/lane\]",
          r"Occupancy \[waves/SIMD\]", "SGPRs Spill", "VGPRs Spill", r"LDS Size \[bytes/block\]")


def remarks(tree, tmp, tag):
    csrc = os.path.join(tree, "pyharp_amd", "csrc")
    procs = []
    for src in sorted(f for f in os.listdir(csrc) if f.endswith(".hip")):
        log = open(os.path.join(tmp, f"{tag}_{src}.txt"), "w")
        cmd = [_build._hipcc(), f"--offload-arch={_build.ARCH}", "-O3", "-std=c++17", "-fPIC",
               "-x", "hip", "-c", src, "-o", os.path.join(tmp, f"{tag}_{src}.o"),
               "-Rpass-analysis=kernel-resource-usage"] + _build.EXTRA.get(src, [])
        procs.append((src, log, subprocess.Popen(cmd, cwd=csrc, stdout=log,
                                                 stderr=subprocess.STDOUT)))
    out = {}
    for src, log, p in procs:
        if p.wait() != 0:
            raise SystemExit(f"{tree}: {src} did not compile, see {log.name}")
        log.close()
        out[src] = parse(log.name)
    return out


def parse(path):
    out, cur = {}, None
    pat = re.compile(r"remark:\s+(" + "|".join(FIELDS) + r"): (\S+)")
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = pat.search(line)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def demangle(name):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt:
        return name
    return subprocess.run([filt, name], capture_output=True, text=True).stdout.strip()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("tree", nargs="?", default=ROOT)
    ap.add_argument("--show", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old, new = remarks(a.parent, tmp, "parent"), remarks(a.tree, tmp, "new")
    total = 0
    for src in sorted(old):
        nd = 0
        for k, v in old[src].items():
            if k not in new.get(src, {}):
                print("MISSING", demangle(k))
                nd += 1
            elif new[src][k] != v:
                print("DIFF", demangle(k), v, new[src][k])
                nd += 1
        total += nd
        print(f"{src}: pre-existing kernels: {len(old[src])} differences: {nd} "
              f"new kernels: {len(set(new.get(src, {})) - set(old[src]))}")
    if a.show:
        for src in sorted(new):
            for k, v in new[src].items():
                n = demangle(k)
                if re.search(a.show, n):
                    print(n.split("(")[0], "V", v.get("VGPRs"), "A", v.get("AGPRs"), "S",
                          v.get("TotalSGPRs"), "scr", v.get("ScratchSize [bytes/lane]"), "occ",
                          v.get("Occupancy [waves/SIMD]"), "vspill", v.get("VGPRs Spill"))
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
