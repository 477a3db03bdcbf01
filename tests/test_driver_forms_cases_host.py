"""The classification of tests/driver_forms_cases.py checked without a GPU: every case's restatement run with M from the setups' own
restatements (the device's factors equal them bit for bit; its AMG hierarchy up to the Lanczos estimate of rho).  The cases named in
NOT_COUNT_CASES are exactly those that miss the class, and every preconditioner keeps its share: two thirds of its cases, one per form."""

import pytest

import driver_forms_cases as C
import driver_restatement as R


@pytest.mark.parametrize("pc", list(C.PCS))
def test_classification_with_the_restatements_factors(pc):
    for case in C.cases_of(pc):
        ref, margin, moved, prefix = C.classify(case, C.cpu_apply(case.pc, case.system))
        assert R.is_count_case(margin, moved) == (case.id in C.COUNT_CASES), (case.id, margin, moved)
        assert prefix >= min(9, len(ref.history)), (case.id, prefix)      # (what a case outside the class is still compared over)
        if case.variant == "atol":
            assert ref.status == R.OK and ref.history[-1] > 0.0, case.id      # the absolute test ends every one of them
            assert ref.updates <= (1 if C.PCS[pc]["capped"] else 1024)
        elif case.variant.startswith("cap") or C.PCS[pc]["capped"]:
            assert ref.status == R.MAX_ITER, case.id          # (a cap is a cap: no capped case converges before it)
        else:
            assert ref.status == R.OK, case.id
    # the guess= sequence, fed the restatement's own solutions
    run = C.GuessRun(pc, C.cpu_apply(pc, C.PCS[pc]["systems"][0]))
    for i in range(C.GUESS_SOLVES):
        bi, x0, ref, margin, moved, prefix = run.step(i)
        if pc == "amg_fp32":
            assert C.guess_id(pc, i) in C.NOT_COUNT_CASES          # (the fp32 cycle: never held to the count rule, GuessRun)
        else:
            assert R.is_count_case(margin, moved) == (C.guess_id(pc, i) in C.COUNT_CASES), (pc, i, margin, moved)
        assert (i == 0) == (not x0.any()) and prefix >= 1
        run.feed(ref.x)
    assert 0.0 < run.dist_x0 <= C.guess_x0_yardstick() / 8.0


def test_shares():
    ids = [c.id for c in C.ALL_CASES]
    assert len(set(ids)) == len(ids) and C.NOT_COUNT_CASES <= set(ids) | C.GUESS_IDS
    for group, pcs in C.GROUPS.items():
        cases = [c for pc in pcs for c in C.cases_of(pc)]
        count = [c for c in cases if c.id in C.COUNT_CASES]
        assert 3 * len(count) >= 2 * len(cases), (group, len(count), len(cases))
        # one count case per way a call can be routed: default flags, the launches forced, a reordered handle, a cap
        for kind in ("plain_or_x0", "launches", "rcm", "cap"):
            of_kind = [c for c in cases if (kind == "launches" and "NO_SMALL" in C.variant_kw(c.variant)["flags"])
                       or (kind == "rcm" and c.reorder) or (kind == "cap" and c.variant.startswith("cap"))
                       or (kind == "plain_or_x0" and c.variant in ("plain", "x0"))]
            assert not of_kind or any(c.id in C.COUNT_CASES for c in of_kind), (group, kind)
