"""SmoothedAggregation(precision="fp32") beside the fp64 cycle of the same run, on the seven systems of profiles/amg_probe.md.

    python tools/amg_fp32_probe.py [--systems p3_100,...] --out profiles/amg_fp32_probe.jsonl
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o amg32 -- \
        python tools/amg_fp32_probe.py --trace-only --systems p3_100,quadtree_foam,delaunay --out levels.jsonl
    python tools/amg_fp32_probe.py --report OUT/amg32_kernel_trace.csv levels.jsonl --ceiling GBS > profiles/amg_fp32_level0_kernels.jsonl
    python -m pytest tests/test_amg_fp32_gpu.py -q -s > apply.log          # the tests print their d, e and iteration figures
    python tools/amg_fp32_probe.py --render profiles/amg_fp32_probe.jsonl profiles/amg_fp32_level0_kernels.jsonl apply.log \
        > amg_fp32_tables.md               # the tables of profiles/amg_fp32_probe.md (its prose is written by hand around them)

Per system and precision (nu = 1, damped Jacobi, the defaults): us per apply (HIP events around 50 applies, the two precisions
interleaved three times, the median reported), iterations, us per update and ms to the solution (rtol_sq = 1e-8, max_iter = 1024),
and the bytes one cycle moves.  --trace-only runs 51 applies per system and precision (fp64 first) and nothing else; --report reads
level 0's four kernels out of that trace as tools/amg_probe.py does.  Bytes: a matrix entry is 12 B in the fp64 cycle and 8 B in
the fp32 one (value + column), a row pointer 4 B, a work-vector element 8 B or 4 B; level 0's right-hand side and result are 8 B
in both.
"""

import argparse
import csv
import json
import pathlib
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent))
import amg_probe as base  # noqa: E402

PRECISIONS = ("fp64", "fp32")


def _level0_bytes(n, nnz, pn, nc, precision):
    """Bytes of level 0's four kernels (nu = 1): every stream and vector once."""
    e, w = (12.0, 8.0) if precision == "fp64" else (8.0, 4.0)
    return {"pre (x = wD^-1 b, r = b - Ax)": e * nnz + 4.0 * (n + 1) + (8.0 + 3 * w) * n,          # b; dinv, x, r
            "restriction (b_1 = P^T r)": e * pn + 4.0 * (nc + 1) + w * (n + nc),
            "prolongation (x += P x_1)": e * pn + 4.0 * (n + 1) + w * (2 * n + nc),
            "post (x += wD^-1 (b - Ax), <r, z>)": e * nnz + 4.0 * (n + 1) + (16.0 + 2 * w) * n}     # b, z; dinv, x


def _cycle_bytes(info, precision):
    e, w = (12.0, 8.0) if precision == "fp64" else (8.0, 4.0)
    total = 0.0
    for l in range(info.levels - 1):
        n, nnz, pn, nc = info.rows[l], info.nnz[l], info.p_nnz[l], info.rows[l + 1]
        if l == 0:
            total += sum(_level0_bytes(n, nnz, pn, nc, precision).values())
            continue
        total += 2 * (e * nnz + 4.0 * (n + 1) + 4 * w * n)
        total += e * pn + 4.0 * (nc + 1) + w * (n + nc)
        total += e * pn + 4.0 * (n + 1) + w * (2 * n + nc)
    nco = info.rows[-1]
    return total + 8.0 * nco * nco + 2 * w * nco


def _system(D, A):
    return D.CsrSystem(*A, A[0].numel() - 1) if isinstance(A, tuple) else D.CsrSystem.from_any(A)


def probe(name, A, ceiling):
    import deeppreconditioning_amd as D
    from deeppreconditioning_amd import poisson
    S = _system(D, A)
    n = S.n
    b = poisson.rhs(n, 0, device="cuda")
    row = {"system": name, "rows": n, "nnz": S.info()["nnz"], "reordered": S.reordered}
    us = {p: [] for p in PRECISIONS}
    for _ in range(3):                                   # interleaved: drift hits both precisions alike
        for p in PRECISIONS:
            S.set_preconditioner(D.SmoothedAggregation(precision=p))
            us[p].append(base._time_applies(S, n))
    for p in PRECISIONS:
        pc = D.SmoothedAggregation(precision=p)
        S.set_preconditioner(pc)
        info = S.amg_hierarchy()
        t = float(np.median(us[p]))
        nbytes = _cycle_bytes(info, p)
        row[p] = {"levels": info.levels, "level_rows": info.rows, "launches_per_apply": info.launches,
                  "us_per_apply": round(t, 2), "us_per_apply_runs": [round(x, 2) for x in us[p]],
                  "cycle_mbytes": round(nbytes / 1e6, 1), "frac_of_stream_ceiling": round(nbytes / (t * 1e3) / ceiling, 3)}
        row[p].update(base._solve(S, b, pc))
    S.close()
    return row


def level0_report(trace_csv, levels_jsonl, ceiling):
    """Level 0's four kernels per system and precision from a --trace-only trace (the launch order of tools/amg_probe.py's report;
    each system ran 51 fp64 applies, then 51 fp32 applies, the first of each a warm-up)."""
    systems = [json.loads(line) for line in open(levels_jsonl) if line.strip()]
    rows = []
    with open(trace_csv) as f:
        for r in csv.DictReader(f):
            if "k_amg_row" in r["Kernel_Name"] or "k_amg_gemv" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    gemv = [i for i, r in enumerate(rows) if "k_amg_gemv" in r[2]]
    prefix = {"pre": "k_amg_row<0,", "restriction": "k_amg_row<4,", "prolongation": "k_amg_row<3,", "post": "k_amg_row<2,"}
    out = []
    for si, sysinfo in enumerate(systems):
        h = 2 * (sysinfo["levels"] - 1)
        offsets = {"pre": -h, "restriction": -h + 1, "prolongation": h - 1, "post": h}
        n, nnz, pn, nc = sysinfo["rows"][0], sysinfo["nnz"][0], sysinfo["p_nnz"][0], sysinfo["rows"][1]
        for pi, p in enumerate(PRECISIONS):
            seg = 2 * si + pi
            mine = gemv[seg * 51 + 1:(seg + 1) * 51]
            for label, nbytes in _level0_bytes(n, nnz, pn, nc, p).items():
                key = label.split(" ")[0]
                durs = []
                for g in mine:
                    kname = rows[g + offsets[key]][2].replace(" ", "")
                    assert prefix[key] in kname and (("float" in kname) == (p == "fp32")), (label, p, kname)
                    durs.append(rows[g + offsets[key]][1])
                t = float(np.median(durs)) / 1e3
                out.append({"system": sysinfo["system"], "precision": p, "kernel": label, "us": round(t, 2),
                            "mbytes": round(nbytes / 1e6, 1), "gbs": round(nbytes / (t * 1e3), 1),
                            "frac_of_ceiling": round(nbytes / (t * 1e3) / ceiling, 3)})
    return out


def _test_tables(log):
    """The `fp32 apply` / `fp32 solve` lines tests/test_amg_fp32_gpu.py prints, as tables."""
    import re
    md = ["", "| system | smoother | d = \\|M_dev x - vcycle32\\| / \\|vcycle32\\| | e = \\|vcycle32 - vcycle\\| / \\|vcycle\\| |", "|---|---|---|---|"]
    solves = ["", "| system | smoother | iterations fp32 / fp64 / restated fp32 | \\|b - A x\\| at rtol_sq = 1e-20, fp32 / fp64 |", "|---|---|---|---|"]
    for line in open(log):
        m = re.search(r"fp32 apply (\S+) (\S+) (\{.*\}): d = (\S+)\s+e = (\S+)", line)
        if m:
            md.append(f"| {m.group(1)} | {m.group(2)} {m.group(3)} | {m.group(4)} | {m.group(5)} |")
        m = re.search(r"fp32 solve (\S+) (\S+): iterations fp32 (\d+), fp64 (\d+), restated fp32 (\d+); .*: fp32 (\S+) .*fp64 (\S+) ", line)
        if m:
            solves.append(f"| {m.group(1)} | {m.group(2)} | {m.group(3)} / {m.group(4)} / {m.group(5)} | {m.group(6)} / {m.group(7)} |")
    return md + solves


def render(probe_jsonl, kernels_jsonl=None, test_log=None):
    lines = [json.loads(line) for line in open(probe_jsonl) if line.strip()]
    ceiling = next(r["stream_ceiling_gbs"] for r in lines if "stream_ceiling_gbs" in r)
    md = ["| system | rows | levels | launches | us / apply fp64 | fp32 | ratio | cycle MB fp64 / fp32 | its fp64 / fp32 | "
          "us per update fp64 / fp32 | ms to solution fp64 / fp32 |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in lines:
        if "system" not in r:
            continue
        if "error" in r:
            md.append(f"| {r['system']} | error: {r['error']} |")
            continue
        a, b = r["fp64"], r["fp32"]
        md.append(f"| {r['system']}{' (reordered)' if r['reordered'] else ''} | {r['rows']:,} | {a['levels']} | {a['launches_per_apply']} | "
                  f"{a['us_per_apply']:.0f} | {b['us_per_apply']:.0f} | {a['us_per_apply'] / b['us_per_apply']:.2f} | "
                  f"{a['cycle_mbytes']:.0f} / {b['cycle_mbytes']:.0f} | {a['iterations']} / {b['iterations']} | "
                  f"{a['us_per_update']:.1f} / {b['us_per_update']:.1f} | {a['ms_to_solution']:.2f} / {b['ms_to_solution']:.2f} |")
    md.append(f"\nStreaming ceiling (`stream_bench`, triad walked by the whole grid): {ceiling:.0f} GB/s.")
    if kernels_jsonl:
        ks = [json.loads(line) for line in open(kernels_jsonl) if line.strip()]
        md += ["", "| system | level-0 kernel | us fp64 | us fp32 | ratio | MB fp64 / fp32 (ratio) | of ceiling fp64 / fp32 |",
               "|---|---|---|---|---|---|---|"]
        for a in (k for k in ks if k["precision"] == "fp64"):
            b = next(k for k in ks if k["precision"] == "fp32" and k["system"] == a["system"] and k["kernel"] == a["kernel"])
            md.append(f"| {a['system']} | {a['kernel']} | {a['us']:.1f} | {b['us']:.1f} | {a['us'] / b['us']:.2f} | "
                      f"{a['mbytes']:.1f} / {b['mbytes']:.1f} ({a['mbytes'] / b['mbytes']:.2f}) | "
                      f"{a['frac_of_ceiling']:.2f} / {b['frac_of_ceiling']:.2f} |")
    if test_log:
        md += _test_tables(test_log)
    return "\n".join(md)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="p3_100,p3_256,p2_1024,unstructured_3_100,quadtree_foam,quadtree_random,delaunay")
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--report", nargs=2, metavar=("KERNEL_TRACE_CSV", "LEVELS_JSONL"), help="level-0 kernels of a --trace-only trace")
    ap.add_argument("--ceiling", type=float, default=None, help="GB/s (--report)")
    ap.add_argument("--render", nargs="+", metavar="JSONL", help="markdown tables from the probe's JSONL [, --report's, the test log]")
    args = ap.parse_args()
    if args.render:
        print(render(*args.render))
        return 0
    if args.report:
        for row in level0_report(args.report[0], args.report[1], args.ceiling):
            print(json.dumps(row))
        return 0
    import deeppreconditioning_amd as D
    names = args.systems.split(",")
    out = open(args.out, "w") if args.out else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    if args.trace_only:
        for name, A in base._systems(names):
            S = _system(D, A)
            for p in PRECISIONS:
                S.set_preconditioner(D.SmoothedAggregation(precision=p))
                base._time_applies(S, S.n)
            emit({"system": name, **base._level_sizes(S)})
            S.close()
        return 0
    ceiling = D.operators.stream_bench(n_read=2, write=True, out_bytes=1 << 28, repeats=10, walk=True)
    emit({"stream_ceiling_gbs": round(ceiling, 1)})
    for name, A in base._systems(names):
        try:
            row = probe(name, A, ceiling)
        except Exception as exc:          # one system's failure is reported, the others still run
            row = {"system": name, "error": f"{type(exc).__name__}: {exc}"}
        emit(row)
    return 0


if __name__ == "__main__":
    sys.exit(main())
