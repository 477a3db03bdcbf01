#!/usr/bin/env python3
"""Resource usage of every instantiation of a set of kernels, two builds side by side.

Reads the remarks that `hipcc --offload-arch=gfx950 <project flags> --cuda-device-only -Rpass-analysis=kernel-resource-usage -c FILE.hip`
writes to stderr (no GPU needed), one folder of `<file>.remarks` per build:

    python tools/chip_resource_table.py PARENT_DIR HEAD_DIR > profiles/chip_shared_device_resources.csv
    python tools/chip_resource_table.py PARENT_DIR HEAD_DIR --kernels k_ns_,k_df_,k_proj_ --registers-may-move \\
        --pair 'k_ns_(update_r|update_xp)<(\\d+), (\\w+), (\\d)>' 'k_proj_\\1<dpcg::NullBasis<\\2, \\3>, \\4>' ...

--kernels: substrings of the (mangled or demangled) names to list; the default is the whole-chip solve kernels.  --pair REGEX TEMPLATE
(repeatable): a parent kernel whose demangled name matches REGEX is compared with the head kernel named by TEMPLATE (re.sub on the
demangled name without its argument list) -- for kernels a change renames.

Prints one CSV line per kernel instantiation -- VGPRs, AGPRs, SGPRs, scratch bytes, SGPR / VGPR spills, LDS bytes, occupancy of the
parent | of the head | the verdict -- and exits 1 when a verdict is bad or a kernel exists on one side only.  Verdicts: `same`;
`DIFFERENT` (bad); with --registers-may-move a line that differs is `moved` when scratch and spills are no higher, occupancy no lower
and LDS no higher than the parent's, else `WORSE` (bad).
"""
import argparse
import glob
import os
import re
import subprocess
import sys

FIELDS = [("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "Scratch"), ("SGPRs Spill", "SGPRspill"),
          ("VGPRs Spill", "VGPRspill"), ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "Occ")]
KERNELS = "k_pcg_chip,k_l2_gather_probe"
NO_HIGHER, NO_LOWER = ("Scratch", "SGPRspill", "VGPRspill", "LDS"), ("Occ",)


def demangle(names):
    if not names:               # (c++filt without arguments reads stdin)
        return {}
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True, stdin=subprocess.DEVNULL).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def read(folder, kernels):
    """{short demangled name: {field: value}} of the kernels asked for"""
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
    pretty = demangle(sorted(table))
    short = {n: re.sub(r"^void dpcg::\(anonymous namespace\)::|\(.*$", "", pretty[n]).replace("> >", ">>") for n in table}
    return {short[n]: v for n, v in table.items() if any(k in n or k in short[n] for k in kernels)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_dir")
    ap.add_argument("head_dir")
    ap.add_argument("--kernels", default=KERNELS)
    ap.add_argument("--pair", nargs=2, action="append", default=[], metavar=("REGEX", "TEMPLATE"))
    ap.add_argument("--registers-may-move", action="store_true")
    args = ap.parse_args()
    kernels = [k for k in args.kernels.split(",") if k]
    parent, head = read(args.parent_dir, kernels), read(args.head_dir, kernels)
    if not parent and not head:
        print("# no kernel in the remarks of either build: nothing compared")
        return 1

    def head_name(n):
        for regex, template in args.pair:
            if re.fullmatch(regex, n):
                return re.sub(regex, template, n)
        return n

    rows = [(n, head_name(n)) for n in sorted(parent)]
    paired = {hn for _, hn in rows}
    rows += [(None, n) for n in sorted(head) if n not in paired]
    print("kernel," + ",".join("parent_" + f for _, f in FIELDS) + "," + ",".join("head_" + f for _, f in FIELDS) + ",verdict")
    bad = 0
    for pn, hn in rows:
        a, b = parent.get(pn), head.get(hn)
        row_a = [a.get(k, "") if a else "-" for k, _ in FIELDS]
        row_b = [b.get(k, "") if b else "-" for k, _ in FIELDS]
        verdict = "same" if row_a == row_b else "DIFFERENT"
        if verdict == "DIFFERENT" and args.registers_may_move and a and b:
            va, vb = ({f: int(r[i]) for i, (_, f) in enumerate(FIELDS)} for r in (row_a, row_b))
            fine = all(vb[f] <= va[f] for f in NO_HIGHER) and all(vb[f] >= va[f] for f in NO_LOWER)
            verdict = "moved" if fine else "WORSE"
        bad += verdict in ("DIFFERENT", "WORSE")
        label = hn if pn in (None, hn) else "%s -> %s" % (pn, hn)
        print('"%s",%s,%s,%s' % (label, ",".join(row_a), ",".join(row_b), verdict))
    print("# %d instantiations, %d bad" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
