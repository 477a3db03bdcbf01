"""Child process of test_bicgstab_edges_gpu.py::test_later_trips_of_the_vector_passes: DPCG_VEC_GRID (read once per process) holds the
grid of the vector passes to 1 or 3 workgroups, so that the software-pipelined loops of k_bi_pass_p / s / x and the loop of k_bi_tt
take a second and later trips on systems a CPU restates in milliseconds (bicgstab_edge_cases.CHILD).  Runs the K-update short run with
M = I, Jacobi and the explicit CSR M, and once from a nonzero x0; prints one JSON line that the parent holds to the restatement."""
import json
import os
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bicgstab_cases as C  # noqa: E402
import bicgstab_edge_cases as E  # noqa: E402
import deeppreconditioning_amd as D  # noqa: E402

grid = int(os.environ["DPCG_VEC_GRID"])
name = E.CHILD[grid][0]
A, b = C.matrix(name), C.rhs(name)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
out = {"name": name, "runs": {}}
for pre, x0 in [(p, None) for p in C.PRECONDS] + [(E.CHILD_X0_PRE, E.x0_of(name))]:
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner({"none": None, "jacobi": D.Jacobi(), "csr": D.CsrPreconditioner(C.neumann_series_csr(A))}[pre])
    out["vec_grid"] = S.reduction_geometry()["vec_grid"]
    res = S.solve_bicgstab(dev(b), None if x0 is None else dev(x0), rtol_sq=E.RTOL_SQ, max_iter=E.K)
    out["runs"][pre + ("" if x0 is None else "_x0")] = {"iterations": res.iterations, "status": res.status, "final_res": res.final_res,
                                                       "history": res.res_history.tolist(), "x": res.x.cpu().numpy().tolist()}
    S.close()
print(json.dumps(out), flush=True)
