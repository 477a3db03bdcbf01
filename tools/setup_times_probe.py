"""Setup times of the preconditioners the shared setup blocks serve, timed as bench.py's extra workloads time theirs (synchronise,
perf_counter around the attach, synchronise).  One JSON line per process; DPCG_LIBRARY selects the library."""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
import deeppreconditioning_amd as D
from deeppreconditioning_amd import poisson

def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r

out = {"lib": os.environ.get("DPCG_LIBRARY", "tree")}
warm = poisson.poisson_system(3, 64)
warm.set_preconditioner(D.Jacobi())
bw = poisson.rhs(warm.n, 0)
t_end = time.perf_counter() + 0.3
while time.perf_counter() < t_end:
    warm.solve(bw, want_history=False)
warm.close()

s = poisson.poisson_system(3, 100)          # 1 000 000 rows
vals = poisson.poisson_csr(3, 100)[2]
def attach(name, make, refresh=False):
    first, _ = timed(lambda: s.set_preconditioner(make()))       # first attach: new pattern (and module load)
    again = [timed(lambda: s.set_preconditioner(make()))[0] for _ in range(3)]
    out[name] = {"setup_new_pattern_ms": round(first, 3), "setup_ms": round(min(again), 3)}
    if refresh:                                                   # the values-only path after update_values
        r = []
        for _ in range(3):
            s.update_values(vals)
            r.append(timed(lambda: s.set_preconditioner(make()))[0])
        out[name]["setup_same_pattern_ms"] = round(min(r), 3)
attach("ic0_solve", lambda: D.IC0("solve"))
attach("ic0_multicolor_solve", lambda: D.IC0("solve", ordering="multicolor"), refresh=True)
attach("ict_multiply", lambda: D.ICT("multiply", 1, 0.1))
attach("fsai_1", lambda: D.FSAI(level=1), refresh=True)
attach("fsai_2", lambda: D.FSAI(level=2))
attach("block_ic0_4096", lambda: D.BlockIC(blocks=4096, variant="ic0"), refresh=True)
attach("block_dic_boxes", lambda: D.BlockIC(blocks=poisson.subdomain_blocks((100, 100, 100), (7, 7, 7)), variant="dic"))
attach("amg", lambda: D.SmoothedAggregation(), refresh=True)
s.close()
A = poisson.unstructured_like_csr(3, 64, seed=0)
for how in ("rcm", "regions"):
    try:
        ms, S = timed(lambda: D.CsrSystem.from_any(A, reorder=how))
        ms2, S2 = timed(lambda: D.CsrSystem.from_any(A, reorder=how))
        out["create_reorder_" + how] = {"setup_new_pattern_ms": round(ms, 3), "setup_ms": round(ms2, 3)}
        S.close(); S2.close()
    except Exception as e:
        out["create_reorder_" + how] = {"error": repr(e)}
small = poisson.poisson_system(2, 49)
s = small
attach("icholt_2401", lambda: D.ICholT("solve", add_fill_in=1, threshold=0.1))
attach("ilut_2401", lambda: D.ILUT("multiply"))
small.close()
print(json.dumps(out))
