"""The block-Jacobi incomplete Cholesky on the device (dpcg_set_precond_block_ic, D.BlockIC) against its numpy restatement
(tests/block_ic_restatement.py): numbering, factor and apply bit for bit -- both variants, every block shape that takes another
path (a short last block, non-contiguous and sparse ids, sizes that are no multiple of the wave, one block of exactly 4096 rows,
one-row blocks, long rows) -- on plain and reordered handles; PCG counts and histories; reuse across update_values; the errors; the
spectrum; the null-space and deflated drivers; detaching."""

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import block_ic_restatement as R
import deflation_restatement as DR
import nullspace_restatement as NR
from deeppreconditioning_amd import meshes
from deeppreconditioning_amd.poisson import neumann_csr, subdomain_blocks
from oracle import c_oracle as CO
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HIST_RTOL = 1e-10
RTOL_SQ = 1e-8
VARIANTS = ("ic0", "dic")


@pytest.fixture(scope="module")
def D():
    import deeppreconditioning_amd as pkg
    assert torch.cuda.is_available(), "these tests need the GPU"
    pkg._lib.lib()
    return pkg


def _csr(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    A.sort_indices()
    return A


# name -> (matrix, what BlockIC takes as `blocks`)
CASES = {
    "poisson2d_12/64": lambda: (O.poisson2d(12), 64),                                          # a short last block of 16 rows
    "poisson2d_48/3x3": lambda: (O.poisson2d(48), subdomain_blocks((48, 48), (3, 3))),         # non-contiguous ids, 256-row blocks
    "poisson2d_48/1000": lambda: (O.poisson2d(48), 1000),                                      # not a multiple of the wave
    "poisson3d_12/2x2x2": lambda: (O.poisson3d(12), subdomain_blocks((12, 12, 12), (2, 2, 2))),
    "poisson3d_20/3x3x3": lambda: (O.poisson3d(20), subdomain_blocks((20, 20, 20), (3, 3, 3))),   # unequal boxes of 294 / 343 rows
    "poisson2d_64/one": lambda: (O.poisson2d(64), 4096),                                       # exactly 4096 rows, 127 levels
    "quadtree/1000": lambda: (meshes.quadtree_fv_laplacian(150, 5), 1000),
    "quadtree_random/1000": lambda: (meshes.quadtree_fv_laplacian(150, 5, numbering="random"), 1000),
    "delaunay_4000/512": lambda: (meshes.delaunay_laplacian(4000, 0), 512),                    # long rows
    "poisson2d_12/sparse_ids": lambda: (O.poisson2d(12), np.array([7, 3, 1000000, 12])[np.random.default_rng(5).integers(0, 4, 144)]),
    "poisson2d_12/one_row": lambda: (O.poisson2d(12), 3 * np.arange(144)[::-1].copy()),        # n one-row blocks
}
# the smallest shapes the transpose of tril(A_B) sees: one row; a diagonal matrix (every column of the strictly lower part empty)
DEGENERATE_CASES = {
    "one_row/1": lambda: (sp.csr_matrix(np.array([[4.0]])), 1),
    "diagonal_5/2": lambda: (sp.diags(np.arange(1.0, 6.0)), 2),
}
COUNT_CASES = {"poisson2d_12/64": 12, "poisson3d_12/2x2x2": 14, "poisson3d_20/3x3x3": 22}
_SYS, _FAC, _PCG = {}, {}, {}


def system(name):
    if name not in _SYS:
        A, blocks = (CASES.get(name) or DEGENERATE_CASES[name])()
        A = _csr(A)
        ids = R.contiguous_ids(A.shape[0], blocks) if isinstance(blocks, int) else np.asarray(blocks)
        _SYS[name] = (A, blocks, ids)
    return _SYS[name]


def restated(name, variant):
    """(L, perm) of the restatement, computed once and shared."""
    if (name, variant) not in _FAC:
        A, _, ids = system(name)
        _FAC[(name, variant)] = R.factor(A, ids, variant, fast=True)
    return _FAC[(name, variant)]


def restated_pcg(name, variant, b_seed=0):
    if (name, variant) not in _PCG:
        A, _, _ = system(name)
        L, perm = restated(name, variant)
        _, k, hist, x = O.preconditioned_conjugate_gradient(A, O.rhs(A.shape[0], b_seed), R.Apply(L, perm), rtol=RTOL_SQ)
        _PCG[(name, variant)] = (k, hist, x)
    return _PCG[(name, variant)]


def _dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def _factor(S):
    rp, ci, v = S.factor()
    return sp.csr_matrix((v, ci, rp), shape=(S.n, S.n))


def _same_bits(X, Y):
    return (np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(X.data.view(np.uint64), Y.data.view(np.uint64)))


def right_hand_sides(n):
    rng = np.random.default_rng(11)
    zeros = O.rhs(n, 1)
    zeros[rng.random(n) < 0.5] = 0.0
    mixed = O.rhs(n, 2) * 10.0 ** rng.uniform(-8, 8, n)
    return [O.rhs(n, 0), zeros, mixed]


def attached(D, name, variant, reorder=None):
    A, blocks, _ = system(name)
    S = D.CsrSystem.from_any(A, reorder=reorder)
    S.set_preconditioner(D.BlockIC(blocks=blocks, variant=variant))
    return S


def check_factor_and_apply(S, name, variant):
    A, _, ids = system(name)
    L, perm = restated(name, variant)
    colors, dperm = S.precond_ordering()
    info = S.info()
    assert colors == 0 and np.array_equal(dperm, perm)
    assert info["precond"] == 9 and info["precond_nnz"] == L.nnz
    assert _same_bits(_factor(S), L)
    bi = S.block_ic_info()
    sizes = np.unique(ids, return_counts=True)[1]
    assert bi["variant"] == variant and bi["blocks"] == sizes.size and bi["max_block"] == sizes.max()
    assert (bi["levels_lower"], bi["levels_upper"]) == R.block_levels(L, ids)
    assert bi["threads"] == (64 if sizes.max() <= 64 else 128 if sizes.max() <= 512 else 256 if sizes.max() <= 2048 else 512)
    for r in right_hand_sides(S.n):
        z = S.precond_apply(_dev(r)).cpu().numpy()
        assert np.array_equal(z.view(np.uint64), R.apply(L, perm, r, fast=True).view(np.uint64))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_factor_ordering_levels_and_apply(D, name, variant):
    S = attached(D, name, variant)
    assert not S.block_ic_info()["pattern_reused"]
    check_factor_and_apply(S, name, variant)
    S.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(DEGENERATE_CASES))
def test_degenerate_shapes(D, name, variant):
    S = attached(D, name, variant)
    check_factor_and_apply(S, name, variant)
    A, _, _ = system(name)
    assert np.array_equal(_factor(S).data, np.sqrt(A.diagonal()))              # both variants: L = sqrt(D)
    S.close()


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["poisson2d_48/3x3", "quadtree_random/1000", "poisson2d_12/sparse_ids"])
def test_reordered_handle(D, name, variant):
    S = attached(D, name, variant, reorder="rcm")                  # reordered before the attach
    assert S.info()["reordered"]
    check_factor_and_apply(S, name, variant)
    S.close()
    T = attached(D, name, variant)                                 # ... and after it: the factor stays attached, its maps are rebuilt
    T._reorder("rcm")
    assert T.info()["reordered"] and T.info()["precond"] == 9
    check_factor_and_apply(T, name, variant)
    res = T.solve(_dev(O.rhs(T.n, 0)), rtol_sq=RTOL_SQ)
    k, _, _ = restated_pcg(name, variant)
    assert res.status == 0 and abs(res.iterations - k) <= 1
    T.close()


def test_one_block_is_the_global_ic0(D):
    A, _, _ = system("poisson2d_64/one")
    S = attached(D, "poisson2d_64/one", "ic0")
    assert S.block_ic_info()["blocks"] == 1 and S.block_ic_info()["levels_lower"] == 127 and S.block_ic_info()["threads"] == 512
    assert _same_bits(_factor(S), CO.ic0(A))
    T = D.CsrSystem.from_any(A, reorder=None)
    T.set_preconditioner(D.IC0("solve"))
    assert _same_bits(_factor(S), _factor(T))
    for r in right_hand_sides(S.n):
        assert torch.equal(S.precond_apply(_dev(r)), T.precond_apply(_dev(r)))
    S.close()
    T.close()


def true_residual(A, b, x):
    e = b - A @ x
    return (e @ e) / (b @ b)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_pcg(D, name, variant):
    A, _, _ = system(name)
    b = O.rhs(A.shape[0], 0)
    k, hist, _ = restated_pcg(name, variant)
    S = attached(D, name, variant)
    res = S.solve(_dev(b), rtol_sq=RTOL_SQ)
    margin = NR.stop_margin(hist, RTOL_SQ)
    diff = float(np.max(np.abs(res.res_history - hist) / hist)) if len(res.res_history) == len(hist) else np.inf
    true = true_residual(A, b, res.x.cpu().numpy())
    print(f"{name} {variant}: {res.iterations} updates (restatement {k}, margin {margin:.3f}), history differs by {diff:.3e}, true residual {true:.3e}")
    assert res.status == 0
    assert S.reduction_geometry()["rz_kind"] == 9                     # one partial of <r, z> per block
    if name in COUNT_CASES:
        if variant == "ic0":
            assert k == COUNT_CASES[name]
        assert margin >= 1.2, f"the stop margin of this count case shrank to {margin:.3f}"
        assert res.iterations == k
        assert diff <= HIST_RTOL
    else:
        assert true < RTOL_SQ and res.res_history[-1] < RTOL_SQ
        assert abs(res.iterations - k) <= 1
    S.close()


@pytest.mark.parametrize("name,expect", [("poisson2d_48/3x3", (96, 37, 29)), ("poisson3d_20/3x3x3", (46, 22, 15))])
def test_between_jacobi_and_global_ic0(D, name, expect):
    A, _, _ = system(name)
    b = _dev(O.rhs(A.shape[0], 0))
    S = D.CsrSystem.from_any(A, reorder=None)
    counts = []
    for M in (D.Jacobi(), D.BlockIC(blocks=system(name)[1]), D.IC0("solve")):
        S.set_preconditioner(M)
        res = S.solve(b, rtol_sq=RTOL_SQ)
        assert res.status == 0
        counts.append(res.iterations)
    print(f"{name}: Jacobi {counts[0]}, blocked {counts[1]}, global IC(0) {counts[2]}")
    assert counts[0] > counts[1] > counts[2]
    assert all(abs(c - e) <= 1 for c, e in zip(counts, expect))
    S.close()


def test_launch_path_on_a_chip_sized_system(D):
    A = _csr(O.poisson3d(41))
    n = A.shape[0]
    ids = R.contiguous_ids(n, 1024)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.Jacobi())
    assert S.chip_info()["chip_eligible"]                             # the size the whole-chip forms take ...
    S.set_preconditioner(D.BlockIC(blocks=1024))
    assert not S.chip_info()["chip_eligible"] and S.info()["precond"] == 9          # ... but not with this kind
    assert S.block_ic_info()["blocks"] == (n + 1023) // 1024 and S.reduction_geometry()["small_threads"] == 0
    assert not S.reduction_geometry()["team_eligible"]
    L, perm = R.factor(A, ids, "ic0", fast=True)
    b = O.rhs(n, 0)
    z = S.precond_apply(_dev(b)).cpu().numpy()
    assert np.array_equal(z.view(np.uint64), R.apply(L, perm, b, fast=True).view(np.uint64))
    res = S.solve(_dev(b), rtol_sq=RTOL_SQ, max_iter=9)
    _, _, hist, _ = O.preconditioned_conjugate_gradient(A, b, R.Apply(L, perm), rtol=RTOL_SQ, max_iter=9)
    assert len(res.res_history) == len(hist) == 10
    assert np.max(np.abs(res.res_history - hist) / hist) <= HIST_RTOL
    S.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_update_values_reuses_the_symbolic_phase(D, variant):
    name = "poisson3d_12/2x2x2"
    A, blocks, ids = system(name)
    S = attached(D, name, variant)
    rng = np.random.default_rng(4)
    d = rng.uniform(0.5, 2.0, A.shape[0])
    for B in (_csr(3.0 * A), _csr(sp.diags(d) @ A @ sp.diags(d))):             # scaled, perturbed: the same pattern, still SPD
        assert np.array_equal(B.indices, A.indices)
        S.update_values(B.data)
        assert S.info()["precond"] == 0
        S.set_preconditioner(D.BlockIC(blocks=blocks, variant=variant))
        assert S.block_ic_info()["pattern_reused"]
        L, perm = R.factor(B, ids, variant, fast=True)
        assert _same_bits(_factor(S), L)
        r = O.rhs(S.n, 3)
        assert np.array_equal(S.precond_apply(_dev(r)).cpu().numpy(), R.apply(L, perm, r, fast=True))
    S.set_preconditioner(D.BlockIC(blocks=blocks, variant="dic" if variant == "ic0" else "ic0"))      # the other variant: the same symbolic phase
    assert S.block_ic_info()["pattern_reused"]
    other = (ids + 1) // 2
    S.set_preconditioner(D.BlockIC(blocks=other, variant=variant))
    assert not S.block_ic_info()["pattern_reused"]
    assert _same_bits(_factor(S), R.factor(B, other, variant, fast=True)[0])
    S.close()


def _jacobi_solve(S, b):
    res = S.solve(b, rtol_sq=RTOL_SQ, max_iter=6)
    return res.iterations, res.res_history.copy(), res.x.clone()


def _unsorted(A):
    col, val = A.indices.copy(), A.data.copy()
    s = A.indptr[10]
    col[[s, s + 1]], val[[s, s + 1]] = col[[s + 1, s]], val[[s + 1, s]]
    return A.indptr.astype(np.int32), col.astype(np.int32), val


def _indefinite():
    A = _csr(O.poisson2d(12)).tolil()
    A[100, 100] = -1.0
    return _csr(A)


ERRORS = {
    "4097_rows": (lambda: _csr(O.poisson2d(65)), lambda n: np.where(np.arange(n) < 4097, 17, 5), "ERR_INVALID", ("17", "4097")),
    "negative_id": (lambda: _csr(O.poisson2d(12)), lambda n: np.where(np.arange(n) == 77, -2, 1), "ERR_INVALID", ("negative", "77")),
    "indefinite": (_indefinite, lambda n: (143 - np.arange(n)) // 64, "ERR_PIVOT", ("row 100",)),
    "no_diagonal": (lambda: _csr(O.poisson2d(12) - sp.diags(np.where(np.arange(144) == 31, 4.0, 0.0))), lambda n: 64, "ERR_INVALID", ("diagonal", "31")),
}


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", list(ERRORS) + ["unsorted_columns", "wrong_length"])
def test_errors_leave_the_previous_preconditioner(D, case, variant):
    if case == "unsorted_columns":
        A = _csr(O.poisson2d(12))
        S = D.CsrSystem.from_host(*_unsorted(A), 144, reorder=None)
        blocks, status, words = 64, "ERR_INVALID", ("ascending", "row 10")
    elif case == "wrong_length":
        S = D.CsrSystem.from_any(_csr(O.poisson2d(12)), reorder=None)
        blocks, status, words = np.zeros(143, dtype=np.int32), None, ()
    else:
        make, ids_of, status, words = ERRORS[case]
        A = make()
        A.eliminate_zeros()
        S = D.CsrSystem.from_any(A, reorder=None)
        blocks = ids_of(S.n)
    S.set_preconditioner(D.Jacobi(dinv=np.full(S.n, 0.25)))
    b = _dev(O.rhs(S.n, 0))
    before = _jacobi_solve(S, b)
    if status is None:
        with pytest.raises(ValueError):
            S.set_preconditioner(D.BlockIC(blocks=blocks, variant=variant))
    else:
        with pytest.raises(D._lib.DpcgError) as e:
            S.set_preconditioner(D.BlockIC(blocks=blocks, variant=variant))
        print(e.value)
        assert e.value.status == getattr(D._lib, status)
        assert all(w in str(e.value) for w in words)
    assert S.info()["precond"] == D._lib.PRECOND_JACOBI
    with pytest.raises(D._lib.DpcgError):
        S.block_ic_info()
    after = _jacobi_solve(S, b)
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and torch.equal(before[2], after[2])
    S.close()


def test_a_failed_attach_leaves_an_attached_block_factor(D):
    name = "poisson2d_12/64"
    S = attached(D, name, "ic0")
    with pytest.raises(D._lib.DpcgError):
        S.set_preconditioner(D.BlockIC(blocks=np.where(np.arange(144) == 3, -1, 0)))
    check_factor_and_apply(S, name, "ic0")
    with pytest.raises(D._lib.DpcgError):
        S.sptrsv(_dev(O.rhs(144, 0)), upper=False)                   # (dpcg_sptrsv serves kinds 4 and 8 only)
    S.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_spectrum(D, variant):
    name = "poisson2d_12/64"
    A, _, _ = system(name)
    L, perm = restated(name, variant)
    Ld = L.toarray()
    Ap = A.toarray()[np.ix_(perm, perm)]
    Y = np.linalg.solve(Ld, np.linalg.solve(Ld, Ap).T)               # L^-1 (P A P^T) L^-T: similar to M A
    lam = np.linalg.eigvalsh(0.5 * (Y + Y.T))
    S = attached(D, name, variant)
    sb = S.spectrum_bounds()
    print(f"{variant}: lambda in [{sb.lambda_min}, {sb.lambda_max}] +- ({sb.err_min}, {sb.err_max}); dense [{lam[0]}, {lam[-1]}]")
    slack = 1e-12 * lam[-1]
    assert sb.converged
    assert abs(sb.lambda_min - lam[0]) <= sb.err_min + slack and abs(sb.lambda_max - lam[-1]) <= sb.err_max + slack
    lo = (sb.lambda_max - sb.err_max - slack) / (sb.lambda_min + sb.err_min + slack)
    hi = (sb.lambda_max + sb.err_max + slack) / (sb.lambda_min - sb.err_min - slack)
    assert lo <= lam[-1] / lam[0] <= hi
    S.close()


def _device_apply(S):
    L = _factor(S)
    perm = S.precond_ordering()[1]
    return lambda r: R.apply(L, perm, r, fast=True)


@pytest.mark.parametrize("variant", VARIANTS)
def test_nullspace_solve(D, variant):
    A = neumann_csr((16, 16))
    n = A.shape[0]
    Z, b = NR.constant(n), np.random.default_rng(1).random(n)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.BlockIC(blocks=subdomain_blocks((16, 16), (4, 4)), variant=variant))
    S.set_nullspace("constant")
    res = S.solve(_dev(b), rtol_sq=RTOL_SQ)
    status, k, hist, x = NR.pcg(A, b, Z, _device_apply(S), rtol_sq=RTOL_SQ)
    print(f"null space {variant}: {res.iterations} updates (restatement {k}, margin {NR.stop_margin(hist, RTOL_SQ):.3f})")
    assert status == NR.OK and res.status == 0 and res.iterations == k
    assert NR.true_residual(A, b, Z, res.x.cpu().numpy()) <= 2.0 * NR.true_residual(A, b, Z, x)
    S.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_deflated_solve(D, variant):
    A = DR.poisson((40, 40))
    n = A.shape[0]
    b = np.random.default_rng(1).random(n)
    V, _ = DR.low_eigenvectors(A, 8, True)
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.BlockIC(blocks=subdomain_blocks((40, 40), (4, 4)), variant=variant))
    S.set_deflation(V[:, :3])
    d = S.deflation()
    res = S.solve(_dev(b), rtol_sq=RTOL_SQ)
    status, k, hist, _ = DR.pcg(A, b, d["W"], d["AW"], _device_apply(S), rtol_sq=RTOL_SQ)
    print(f"deflated {variant}: {res.iterations} updates (restatement {k}, margin {NR.stop_margin(hist, RTOL_SQ):.3f})")
    assert status == DR.OK and res.status == 0 and res.iterations == k
    assert DR.true_residual(A, b, res.x.cpu().numpy()) < RTOL_SQ
    S.close()


def test_detaching_restores_the_plain_solve(D):
    A, blocks, _ = system("poisson2d_48/3x3")
    b = _dev(O.rhs(A.shape[0], 0))
    S = D.CsrSystem.from_any(A, reorder=None)
    S.set_preconditioner(D.BlockIC(blocks=blocks))
    assert S.solve(b, rtol_sq=RTOL_SQ).status == 0
    S.set_preconditioner(D.Jacobi())
    with pytest.raises(D._lib.DpcgError):
        S.block_ic_info()
    T = D.CsrSystem.from_any(A, reorder=None)
    T.set_preconditioner(D.Jacobi())
    rs, rt = S.solve(b, rtol_sq=RTOL_SQ), T.solve(b, rtol_sq=RTOL_SQ)
    assert rs.iterations == rt.iterations and np.array_equal(rs.res_history, rt.res_history) and torch.equal(rs.x, rt.x)
    S.close()
    T.close()
