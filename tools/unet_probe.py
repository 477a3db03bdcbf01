"""PreconditionerSparseUNet forward with the harness's channels [1,16,32,64,32,16,1] on 2-D Poisson (4 096, 65 536 and 262 144
rows, batch 1 and 4, seeded random weights): the HIP path (unet_hip.py, csrc/dpcg_unet.hip) against the torch restatement
(extras_unet.py, forced by DPCG_CNN_TORCH=1 -- the path every U-Net forward took before the HIP one existed).

Times are medians over --reps calls after --warmup calls, each call bracketed by torch.cuda.synchronize() and timed on the
host: what the harness's `setups` column sees.
  torch          the torch restatement
  hip_new        a new pattern on a new plan: plan create (device allocations) + forward
  hip_rebuild    a new pattern on a recycled plan (three index tensors in turn, two plans cached): rebuild + forward
  hip_cached     the cached plan: forward only

    python tools/unet_probe.py [--out FILE.jsonl]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o unet -- python tools/unet_probe.py --trace-workload COST.json
    python tools/unet_probe.py --layers OUT/.../unet_kernel_trace.csv --cost COST.json
The last form needs no GPU: it splits the trace into forwards (16 convolution kernels, then k_unet_out) and reports every
layer's median time and its achieved fraction of the fp32 matrix peak and of HBM by `unet_forward_cost`."""

from __future__ import annotations

import argparse
import csv
import json
import os
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HARNESS = [1, 16, 32, 64, 32, 16, 1]
SIZES = (64, 256, 512)           # 4 096, 65 536, 262 144 rows
BATCHES = (1, 4)
TRACE_FORWARDS = 5               # cached forwards per configuration in --trace-workload
PEAK_FP32_MATRIX = 256 * 4 * 64 * 2.4e9     # CUs x SIMDs x FLOP/clk (v_mfma_f32_16x16x4_f32) x 2.4 GHz = 157 TFLOP/s
PEAK_HBM = 8.0e12                           # MI355X HBM3E, bytes/s


def _setup(n, batch):
    import torch
    from deeppreconditioning_amd import model as M
    from oracle import oracle as O
    torch.manual_seed(69)
    net = M.PreconditionerSparseUNet(HARNESS).cuda()
    inp, _ = M.tril_batch_from_csr([O.poisson2d(n)] * batch, device="cuda")
    return net, inp


def _median_ms(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def measure(args):
    import torch
    from deeppreconditioning_amd.utils import SparseBatch
    rows = []
    with torch.no_grad():
        for n in SIZES:
            for batch in BATCHES:
                net, inp = _setup(n, batch)
                copies = [SparseBatch(inp.features, inp.indices.clone(), inp.spatial_shape, inp.batch_size) for _ in range(3)]
                turn = [0]

                def new_plan():
                    net.__dict__.pop("_hip_unet_plans", None)
                    net(inp)

                def rebuild():
                    turn[0] += 1
                    net(copies[turn[0] % 3])

                r = {"rows": n * n, "batch": batch, "sites": int(inp.indices.shape[0])}
                r["hip_new_ms"] = _median_ms(new_plan, args.warmup, args.reps)
                r["hip_rebuild_ms"] = _median_ms(rebuild, args.warmup, args.reps)
                r["hip_cached_ms"] = _median_ms(lambda: net(inp), args.warmup, args.reps)
                os.environ["DPCG_CNN_TORCH"] = "1"
                try:
                    r["torch_ms"] = _median_ms(lambda: net(inp), args.warmup, args.reps)
                finally:
                    del os.environ["DPCG_CNN_TORCH"]
                r["speedup_new"] = r["torch_ms"] / r["hip_new_ms"]
                r["speedup_cached"] = r["torch_ms"] / r["hip_cached_ms"]
                print(json.dumps(r), flush=True)
                rows.append(r)
                del net, inp, copies
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


def trace_workload(cost_path):
    """One plan + TRACE_FORWARDS cached forwards per configuration, in the order of SIZES x BATCHES; the cost model of each
    into `cost_path`."""
    import torch
    from deeppreconditioning_amd import model as M
    costs = []
    with torch.no_grad():
        for n in SIZES:
            for batch in BATCHES:
                net, inp = _setup(n, batch)
                net(inp)
                for _ in range(TRACE_FORWARDS):
                    net(inp)
                torch.cuda.synchronize()
                costs.append({"rows": n * n, "batch": batch, "cost": M.unet_forward_cost(net, inp)})
                del net, inp
                torch.cuda.empty_cache()
    with open(cost_path, "w") as f:
        json.dump(costs, f)


def layers(trace_csv, cost_path):
    costs = json.load(open(cost_path))
    with open(trace_csv) as f:
        ks = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f)
              if "k_unet_conv" in r["Kernel_Name"] or "k_unet_out" in r["Kernel_Name"]]
    ks.sort(key=lambda k: k[1])
    forwards, cur = [], []
    for k in ks:
        cur.append(k)
        if "k_unet_out" in k[0]:
            forwards.append(cur)
            cur = []
    per = 1 + TRACE_FORWARDS
    assert len(forwards) == per * len(costs), (len(forwards), len(costs))
    for ci, c in enumerate(costs):
        runs = forwards[ci * per + 1:(ci + 1) * per]              # the cached forwards
        print(f"\n{c['rows']} rows x batch {c['batch']}:")
        print(f"| layer | C_in -> C_out | sites | kernel | median us | TFLOP/s | % fp32 matrix peak | GB/s | % HBM |")
        print("|---|---|---|---|---|---|---|---|---|")
        total = 0.0
        for li, lay in enumerate(c["cost"]["layers"]):
            us = statistics.median((run[li][2] - run[li][1]) / 1e3 for run in runs)
            total += us
            full = runs[0][li][0]
            name = full[full.index("k_unet"):].split("(")[0]
            tf = lay["flops"] / (us * 1e-6) / 1e12
            gb = lay["min_hbm_bytes"] / (us * 1e-6) / 1e9
            print(f"| {lay['layer']} | {lay['c_in']} -> {lay['c_out']} | {lay['sites']} | `{name}` | {us:.1f} | {tf:.2f} | "
                  f"{100 * tf * 1e12 / PEAK_FP32_MATRIX:.1f} | {gb:.0f} | {100 * gb * 1e9 / PEAK_HBM:.1f} |")
        f_all, b_all = c["cost"]["flops"], c["cost"]["min_hbm_bytes"]
        print(f"| all (kernel time) | | | | {total:.1f} | {f_all / (total * 1e-6) / 1e12:.2f} | "
              f"{100 * f_all / (total * 1e-6) / PEAK_FP32_MATRIX:.1f} | {b_all / (total * 1e-6) / 1e9:.0f} | "
              f"{100 * b_all / (total * 1e-6) / PEAK_HBM:.1f} |")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--trace-workload", metavar="COST_JSON")
    ap.add_argument("--layers", metavar="TRACE_CSV")
    ap.add_argument("--cost", metavar="COST_JSON")
    a = ap.parse_args()
    if a.layers:
        layers(a.layers, a.cost)
    elif a.trace_workload:
        trace_workload(a.trace_workload)
    else:
        measure(a)
