#!/usr/bin/env python3
"""Per-kernel resources of a librxmatch.so's gfx950 code object (llvm-readelf --notes): VGPRs, AGPRs, SGPRs, scratch bytes,
static LDS bytes, VGPR / SGPR spill counts.  One TSV row per kernel, sorted by name; with two libraries, the rows that differ.
usage: kernel_resources.py LIB [OTHER_LIB]"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import kernel_census as kc  # noqa: E402

KEYS = [".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
        ".vgpr_spill_count", ".sgpr_spill_count"]


def resources(lib):
    with tempfile.TemporaryDirectory() as d:
        names = kc.code_object_kernels(lib, d)
        co = [f for f in os.listdir(d) if f.endswith("gfx950")][0]
        notes = subprocess.run([kc.llvm_tools()[1], "--notes", os.path.join(d, co)], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        block = ".agpr_count" + block
        m = re.search(r"\.name:\s+(\S+)", block)
        if not m or m.group(1) not in names:
            continue
        vals = {}
        for k in KEYS:
            v = re.search(re.escape(k) + r":\s+(\d+)", block)
            vals[k] = int(v.group(1)) if v else -1
        out[names[m.group(1)]] = vals
    return out


def main():
    a = resources(sys.argv[1])
    print("kernel\t" + "\t".join(k.strip(".") for k in KEYS))
    if len(sys.argv) == 2:
        for n in sorted(a):
            print(n + "\t" + "\t".join(str(a[n][k]) for k in KEYS))
        return
    b = resources(sys.argv[2])
    for n in sorted(set(a) | set(b)):
        if a.get(n) != b.get(n):
            print(n + "\t" + "\t".join(f"{a.get(n, {}).get(k)}->{b.get(n, {}).get(k)}" if a.get(n, {}).get(k) != b.get(n, {}).get(k)
                                       else str(a[n][k]) for k in KEYS))


if __name__ == "__main__":
    main()
