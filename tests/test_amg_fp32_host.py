"""CPU checks of the fp32 cycle's contract (tests/amg_fp32_restatement.py) and of SmoothedAggregation's `precision` argument: the
reference side of every condition tests/test_amg_fp32_gpu.py puts on the device."""

import numpy as np
import pytest

import amg_fp32_restatement as R32
import amg_restatement as R
import amg_smoother_restatement as SR
from oracle import oracle as O

# (smoother, sweeps): what the device tests run
CASES = [(SR.JACOBI, 1), (SR.JACOBI, 2), (SR.CHEBYSHEV, 1)]


@pytest.fixture(scope="module")
def system():
    A = O.poisson2d(33)
    H = R.hierarchy(A, max_coarse=50)
    assert len(H.levels) >= 3
    return A, H


def _cycles(H, kind, sweeps):
    sm = SR.smoothers_for(H, kind)
    return (lambda v: SR.vcycle(H, sm, v, sweeps)), (lambda v: R32.vcycle32(H, v, sm, sweeps)), sm


def test_argument_validation():
    from deeppreconditioning_amd import SmoothedAggregation
    assert SmoothedAggregation().precision == "fp64"
    assert SmoothedAggregation(precision="fp32", smoother="chebyshev").precision == "fp32"
    with pytest.raises(ValueError):
        SmoothedAggregation(precision="fp16")
    with pytest.raises(ValueError):
        SmoothedAggregation(precision="fp32", smoother="gauss_seidel")


def test_default_arguments_are_the_jacobi_cycle(system):
    _, H = system
    v = O.rhs(H.levels[0].A.shape[0], 5)
    assert np.array_equal(R32.vcycle32(H, v), R32.vcycle32(H, v, SR.smoothers_for(H, SR.JACOBI), 1))
    assert np.array_equal(R32.VCycle32(H) @ v, R32.vcycle32(H, v))


@pytest.mark.parametrize("kind,sweeps", CASES)
def test_restated_cycle_is_symmetric_up_to_its_roundings(system, kind, sweeps):
    _, H = system
    _, m32, _ = _cycles(H, kind, sweeps)
    rng = np.random.default_rng(3)
    n = H.levels[0].A.shape[0]
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    Mx, My = m32(x), m32(y)
    assert abs(x @ My - y @ Mx) <= 1e-5 * np.linalg.norm(Mx) * np.linalg.norm(y)


@pytest.mark.parametrize("kind,sweeps", CASES)
def test_size_of_the_rounding_effect(system, kind, sweeps):
    _, H = system
    m64, m32, _ = _cycles(H, kind, sweeps)
    x = np.random.default_rng(3).standard_normal(H.levels[0].A.shape[0])
    ref = m64(x)
    e = np.linalg.norm(m32(x) - ref) / np.linalg.norm(ref)
    print(f"{kind} sweeps={sweeps}: e = {e:.3e}")
    assert 0.0 < e <= 1e-5


@pytest.mark.parametrize("kind,sweeps", CASES)
def test_pcg_count(system, kind, sweeps):
    A, H = system
    sm = SR.smoothers_for(H, kind)
    b = O.rhs(A.shape[0], 0)
    _, it64, _, _ = O.preconditioned_conjugate_gradient(A, b, SR.VCycle(H, sm, sweeps), rtol=1e-8)
    _, it32, _, x = O.preconditioned_conjugate_gradient(A, b, R32.VCycle32(H, sm, sweeps), rtol=1e-8)
    print(f"{kind} sweeps={sweeps}: iterations fp64 {it64}, fp32 {it32}")
    assert abs(it32 - it64) <= 1
    assert np.linalg.norm(b - A @ x) <= 1e-3 * np.linalg.norm(b)
