#!/usr/bin/env python3
"""Resource usage of every instantiation of the whole-chip solve kernels, two builds side by side.

Reads the remarks that `hipcc --offload-arch=gfx950 <project flags> --cuda-device-only -Rpass-analysis=kernel-resource-usage -c FILE.hip`
writes to stderr (no GPU needed), one folder of `<file>.remarks` per build:

    python tools/chip_resource_table.py PARENT_DIR HEAD_DIR > profiles/chip_shared_device_resources.csv

Prints one CSV line per kernel instantiation -- VGPRs, AGPRs, SGPRs, scratch bytes, SGPR / VGPR spills, LDS bytes, occupancy of the
parent | of the head | same / DIFFERENT -- and exits 1 when any line differs or a kernel exists on one side only.
"""
import glob
import os
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "Scratch"), ("SGPRs Spill", "SGPRspill"),
          ("VGPRs Spill", "VGPRspill"), ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "Occ")]
KERNELS = ("k_pcg_chip", "k_l2_gather_probe")


def demangle(names):
    if not names:               # (c++filt without arguments reads stdin)
        return {}
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True, stdin=subprocess.DEVNULL).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def read(folder):
    table = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.remarks"))):
        name = None
        for line in open(path):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                table[name] = {}
                continue
            m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
            if m and name:
                table[name][m.group(1)] = m.group(2)
    return table


def main():
    parent, head = read(sys.argv[1]), read(sys.argv[2])
    names = sorted(n for n in set(parent) | set(head) if any(k in n for k in KERNELS))
    if not names:
        print("# no kernel in the remarks of either build: nothing compared")
        return 1
    pretty = demangle(names)
    print("kernel," + ",".join("parent_" + f for _, f in FIELDS) + "," + ",".join("head_" + f for _, f in FIELDS) + ",verdict")
    bad = 0
    for n in names:
        a, b = parent.get(n), head.get(n)
        row_a = [a.get(k, "") if a else "-" for k, _ in FIELDS]
        row_b = [b.get(k, "") if b else "-" for k, _ in FIELDS]
        same = row_a == row_b
        bad += 0 if same else 1
        short = re.sub(r"^void dpcg::\(anonymous namespace\)::|\(.*$", "", pretty[n])
        print('"%s",%s,%s,%s' % (short, ",".join(row_a), ",".join(row_b), "same" if same else "DIFFERENT"))
    print("# %d instantiations, %d differ" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
