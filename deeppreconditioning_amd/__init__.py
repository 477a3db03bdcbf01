"""MI355X-native preconditioned-CG solve path with the API of uibk.deep_preconditioning.

    from deeppreconditioning_amd.cg import preconditioned_conjugate_gradient

The solver kernels live in `csrc/` (HIP, gfx950) behind the C ABI of `include/dpcg.h`.
"""

from . import _lib  # noqa: F401
from .operators import (FSAI, IC0, ILU0, BlockIC, ICT, ILUT, ICholT, AmgHierarchy, CsrPreconditioner, CsrSystem, Identity, Jacobi, LLtMultiply, LLtSolve,  # noqa: F401
                        OperatorPreconditioner, Preconditioner, ProjectedGuess, RefinedSolveResult, SmoothedAggregation, SolveResult, SpectrumBounds, as_preconditioner,
                        csr_arrays, dot)

__all__ = ["CsrSystem", "Preconditioner", "Identity", "Jacobi", "CsrPreconditioner", "LLtMultiply", "LLtSolve", "IC0", "ICT", "ICholT", "ILUT", "ILU0", "FSAI", "BlockIC", "OperatorPreconditioner",
           "SmoothedAggregation", "AmgHierarchy", "ProjectedGuess", "SolveResult", "RefinedSolveResult", "SpectrumBounds", "as_preconditioner", "csr_arrays", "dot"]
