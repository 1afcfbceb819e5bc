"""T4 (GPU): whole fits under solve_dtype="refine" against the reference fixtures, at the band of the default path
(tests/test_gpu_parity.py: TOL).  The fixtures are the ones whose rows "auto" redoes in fp64: lambda = 1e-2 and 1e-4 at
k = 64, the mid-rank k = 64 fixture and the full k = 128 one.  What share of the flagged rows the refinement keeps is
printed and recorded, not asserted: only that the mode is used at all."""
import pytest

from tests.common import Golden, model_for
from tests.gpu_common import record_margins
from tests.test_gpu_parity import TOL, _check_against_fixture, _cuda, _tol_for

pytestmark = pytest.mark.gpu

FIXTURES = ("g11_lam1e-2_k64", "g11_lam1e-4_k64", "g9_k64_mid", "g10_full_k128")


@pytest.mark.parametrize("name", FIXTURES)
def test_refine_fit_matches_reference_fixture(name, monkeypatch):
    _cuda()
    from collaborative_filtering_amd.backend import HipBackend
    seen = {"calls": 0, "flagged": 0, "fallback": 0, "steps": [0] * 9}
    inner = HipBackend.row_solve

    def counted(self, **kw):
        inner(self, **kw)
        if self.solve_dtype == "refine" and self.cond_limit > 0.0 and not kw.get("f64"):
            seen["calls"] += 1
            seen["flagged"] += int(self._redo_count.item())
            seen["fallback"] += int(self._fallback_count.item())
            seen["steps"] = [a + int(b) for a, b in zip(seen["steps"], self._refine_steps.tolist())]

    monkeypatch.setattr(HipBackend, "row_solve", counted)
    g = Golden(name)
    model = model_for(g, solve_dtype="refine")
    r, c, v = g.train
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"],
                  min_iters=g.cfg["min_iters"], verbose=0)
    accepted = sum(seen["steps"])
    print(f"{name}: row_solve calls {seen['calls']} flagged {seen['flagged']} accepted {accepted} "
          f"fallback {seen['fallback']} steps {seen['steps']}")
    record_margins(f"refine fit {name}", dict(seen, accepted=accepted))
    assert model._eng.be.solve_dtype == "refine" and seen["calls"] > 0
    assert seen["flagged"] >= accepted + seen["fallback"] >= 0
    _check_against_fixture(model, g, _tol_for(name, TOL))
