#!/usr/bin/env python
"""The mutant table of profiles/coo_edges.md: how far the numpy restatement of the training-path COO operators
(tests/coo_restatement.py) with ONE defect built in lies from the true one, in units of the a-priori bound gamma_m S the GPU results
are held to (tests/test_coo_edges_gpu.py), on the cases of tests/coo_edge_cases.py.  CPU only.

    python tools/coo_edges_probe.py          # rewrites the section between the `mutants` markers, leaves the rest of the file
"""

import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import coo_edge_cases as C  # noqa: E402

PROFILE = ROOT / "profiles" / "coo_edges.md"
BEGIN, END = "<!-- mutants: begin -->", "<!-- mutants: end -->"


def smallest_distance(name, op, which):
    """over both transposes and every width of the case: the smallest distance, i.e. the comparison that shows the mutant least"""
    c = C.case(name)
    found = []
    for ncols in (c.widths if op in ("spmm", "sddmm") else (0,)):
        for transpose in C.TRANSPOSES:
            other = C.mutated(name, op, transpose, ncols, which)
            if other is not None:
                far = C.distance(C.restated(name, op, transpose, ncols), other)
                if which != C.MUTANTS[2] or far > 0:         # (the last triple of out_of_range is one out of range: nothing to drop)
                    found.append(far)
    return min(found) if found else None


def section():
    lines = [BEGIN, "## Mutants of the restatement", "",
             "Distance of the restatement with one defect from the true one, in bounds gamma_m S of the true one (`inf`: an output whose "
             "bound is 0 -- one product, or nothing at all -- differs); the smallest over both `transpose` values and the case's panel "
             "widths.  `-`: the case cannot show the defect.  The large cases are mutated on the operator they are there for.  "
             "tests/test_coo_edges_host.py asks >= 10 on the cases it names.", ""]
    for which in C.MUTANTS:
        lines += [f"### {which}", "", "| case | spmv | edge | spmm | sddmm |", "|---|---|---|---|---|"]
        for name in C.CASES:
            cells = []
            for op in C.OPS:
                far = smallest_distance(name, op, which) if op in C.MUTANT_OPS.get(name, C.OPS) else None
                cells.append("-" if far is None else f"{far:.3g}")
            if any(cell != "-" for cell in cells):
                lines.append(f"| {name} | " + " | ".join(cells) + " |")
        lines.append("")
    lines += ["### an unstable sort in COO -> CSR (equal keys back to front)", "",
              "COO -> CSR is compared bit for bit, so every difference counts.", "",
              "| case | entries | unique | sums that differ | largest difference |", "|---|---|---|---|---|"]
    for name in C.COO_CASES:
        stable, unstable = C.coo_restated(name), C.coo_restated(name, stable=False)
        differ = stable[2] != unstable[2]
        lines.append(f"| {name} | {len(C.coo_case(name)[0])} | {len(differ)} | {int(differ.sum())} | "
                     f"{np.abs(stable[2] - unstable[2]).max(initial=0.0):.3g} |")
    lines += ["", END]
    return "\n".join(lines)


def main():
    text = PROFILE.read_text() if PROFILE.exists() else f"# The training-path COO kernels and COO -> CSR at their edges\n\n{BEGIN}\n{END}\n"
    head, rest = text.split(BEGIN, 1)
    PROFILE.write_text(head + section() + rest.split(END, 1)[1])
    print(f"wrote {PROFILE}")


if __name__ == "__main__":
    main()
