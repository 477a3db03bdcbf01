"""CPU checks of the smoothed-aggregation contract (tests/amg_restatement.py) and of SmoothedAggregation's argument validation."""

import numpy as np
import pytest
import scipy.sparse as sp

import amg_restatement as R
from oracle import oracle as O


def _laplacian_1d(n):
    return sp.diags([-np.ones(n - 1), 2 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1]).tocsr()


def test_splitmix_matches_the_lanczos_start_hash():
    # the top 53 bits of h(seed, i), scaled to [-1, 1), are the Lanczos start vector's entries (dpcg_lanczos.hip, k_lz_start)
    h = R.splitmix(0, np.arange(4))
    v = (h >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0) * 2.0 - 1.0
    assert np.all(np.abs(v) < 1.0) and len(set(h.tolist())) == 4
    assert R.splitmix(7, np.arange(3)).tolist() != R.splitmix(8, np.arange(3)).tolist()


def test_aggregates_of_a_1d_laplacian():
    A = _laplacian_1d(16)
    S = R.strength(A)
    roots = R.mis2(S, 0)
    # derived by hand from the rules: the roots (hash order, seed 0) are >= 3 apart; 1 and 3, 5, 8 and 10, 11 and 13, 14 join the
    # root next to them; 2 sits between the step-1-assigned 1 and 3 at equal |a_ij| and goes to the smaller index (aggregate 0);
    # 6 has one step-1-assigned neighbour, 5 (7 is not adjacent to a root), and joins its aggregate 1; 7 joins 8's aggregate 2
    assert np.nonzero(roots)[0].tolist() == [0, 4, 9, 12, 15]
    assert R.aggregate(A, S, roots).tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4]


def test_aggregates_of_a_5x5_grid():
    A = O.poisson2d(5)
    S = R.strength(A)
    roots = R.mis2(S, 0)
    assert np.nonzero(roots)[0].tolist() == [0, 9, 11, 20, 23]
    agg = R.aggregate(A, S, roots).reshape(5, 5)
    assert agg.tolist() == [[0, 0, 0, 1, 1],
                            [0, 2, 2, 1, 1],
                            [2, 2, 2, 1, 1],
                            [3, 2, 2, 4, 1],
                            [3, 3, 4, 4, 4]]


def test_mis2_is_a_distance_two_maximal_independent_set():
    A = O.unstructured_like(O.poisson2d(30), seed=2)
    S = R.strength(A)
    roots = R.mis2(S, 5)
    G = (S + sp.eye(S.shape[0])).tocsr()
    G.data[:] = 1
    G2 = (G @ G).tocsr()
    r = np.nonzero(roots)[0]
    B = G2[r][:, r].tocoo()
    assert np.all(B.row == B.col)                                         # independent at distance 2
    assert np.all(np.asarray(G2[:, r].sum(axis=1)).ravel() > 0)          # maximal: every node within two hops of a root


def test_strength_theta_drops_weak_connections():
    A = sp.csr_matrix(np.array([[4.0, -1.0, -0.01], [-1.0, 4.0, 0.0], [-0.01, 0.0, 4.0]]))
    assert R.strength(A, 0.0).nnz == 4             # the explicit zero is not a connection
    assert R.strength(A, 0.1).nnz == 2


def test_vcycle_is_symmetric_positive_definite():
    for A in (O.poisson2d(16), O.unstructured_like(O.poisson2d(14), seed=1)):
        H = R.hierarchy(A, max_coarse=10)
        assert len(H.levels) >= 3
        M = R.dense_operator(H)
        assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
        assert np.linalg.eigvalsh((M + M.T) / 2).min() > 0


def test_iterations_grow_far_slower_than_jacobi():
    its = {}
    for m in (32, 256):
        A = O.poisson2d(m)
        b = O.rhs(A.shape[0], 0)
        _, it_sa, _, _ = O.preconditioned_conjugate_gradient(A, b, R.VCycle(R.hierarchy(A)))
        _, it_j, _, _ = O.preconditioned_conjugate_gradient(A, b, sp.diags(1.0 / A.diagonal()))
        its[m] = (it_sa, it_j)
    growth_sa = its[256][0] / its[32][0]
    growth_j = its[256][1] / its[32][1]
    assert growth_j > 6
    assert growth_sa < 0.5 * growth_j, its


@pytest.mark.parametrize("kw", [dict(theta=-0.1), dict(theta=1.5), dict(max_levels=0), dict(max_levels=65), dict(max_coarse=0),
                                dict(sweeps=0), dict(sweeps=9), dict(seed=-1)])
def test_smoothed_aggregation_rejects_bad_arguments(kw):
    from deeppreconditioning_amd import SmoothedAggregation
    with pytest.raises(ValueError):
        SmoothedAggregation(**kw)


def test_smoothed_aggregation_needs_the_system():
    from deeppreconditioning_amd import SmoothedAggregation
    with pytest.raises(TypeError):
        SmoothedAggregation() @ np.ones(4)


def test_harness_knows_the_technique_and_keeps_its_defaults():
    from deeppreconditioning_amd.benchmark_suite import COMPARABILITY, BenchmarkSuite
    assert "algebraic_multigrid" in COMPARABILITY
    assert "algebraic_multigrid" not in BenchmarkSuite.__dataclass_fields__["techniques"].default
