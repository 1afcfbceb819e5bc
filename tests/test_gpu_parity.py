"""T3/T4 (GPU): the HIP path through the C ABI against the golden fixtures from
the real reference and against the CPU oracle.

Stated tolerances of the fp32 path (reference is float64 end to end; the HIP path stores factors in fp32
and accumulates Gram / Cholesky in fp32, statistics in fp64).  They are set above the error observed on the
MI355X over all fixtures and both Gram modes (profiles/parity_margins.py -> profiles/r03_parity_margins.json,
default path: history <= 2.5e-7, factors <= 1.8e-5 of max|ref|, biases <= 4.5e-7, mu <= 1.5e-7, W <= 2.8e-5 of
max|ref|, predictions <= 8.6e-5, fold test RMSE <= 2.0e-7) - 3x to 10x above them:
  train-RMSE history         |d| <= 2e-6        (budget in BASELINE.json: 1e-4)
  U/V/b_u/b_i norm series    rtol 2e-6
  fold-0 test RMSE           |d| <= 1e-6
  factors U, V, W            rtol 1e-4, atol 5e-5 * max|ref|
  biases                     atol 5e-6;  mu atol 1e-6
  predictions at the fold    atol 3e-4
  iteration count (early stop) identical
The DEFAULT path (solve_dtype="auto") holds these on every fixture, including lambda = 1e-2 and 1e-4 with
rank-deficient rows (scripts/tune_params.py:100-101 searches lambda in [1e-4, 1e4]): rows whose condition estimate
exceeds the limit are redone in fp64 inside the same als_row_solve call, and with lambda_w + 1e-10 < 1e-2 the V-step
by-products, the sweep and the W-step accumulate in fp64.  There are no per-fixture overrides for it except the
documented band of the one fixture that is ill-conditioned as a PROBLEM (g12_wlam0_k80, TOL_ILL_POSED below).
solve_dtype="float32" (every row in fp32 whatever its conditioning) is tested against TOL_FP32_ONLY: lambda = 1e-2
inside the 1e-4 budget but outside the tight band, lambda = 1e-4 outside the budget (that is what "auto" is for).
"""
import os
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.common import Golden, golden_names, model_for


def _cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no ROCm device is visible")
    return torch


TOL = dict(hist=2e-6, norms=2e-6, test_rmse=1e-6, f_rtol=1e-4, f_atol=5e-5, bias=5e-6, mu=1e-6, pred=3e-4)
# solve_dtype="float32" ONLY (every row in fp32 whatever its conditioning); keyed by fixture.  None = outside the 1e-4
# budget in fp32 (documented, not asserted).  The default (solve_dtype="auto") has no overrides: rows whose condition
# estimate exceeds the limit are redone in fp64 by the same call.
TOL_FP32_ONLY = {
    "g11_lam1e-2_k64": dict(hist=1e-4, norms=1e-3, test_rmse=1e-4, f_rtol=0.0, f_atol=1e-2, bias=2e-4, mu=1e-6, pred=2e-2),
    "g11_lam1e-4_k64": None,
}


# solve_dtype="float64": what is left is the fp32 storage of U, V, b between half-steps (and, with features / the
# Laplacian, the fp32 item Grams of the W-step and the fp32 triangular solves of the sweep).  Observed over all
# fixtures: history <= 7e-9, fold test RMSE <= 9e-9, biases <= 6e-8, mu <= 7e-9, factors <= 5.3e-6 of max|ref|.
TOL64 = dict(hist=1e-7, norms=2e-6, test_rmse=1e-7, f_rtol=1e-4, f_atol=5e-5, bias=1e-6, mu=1e-7, pred=5e-5)
# g12_wlam0_k80 (lambda_w = 0, k = 80 on 4000 ratings: |W| ~ 80) is ill-conditioned as a PROBLEM: rounding U, V, b to
# fp32 between the half-steps of the float64 oracle - the product's storage type, nothing else changed - already moves
# its predictions by 2.6e-5 and its fold RMSE by 1.3e-7 (the other fixtures: 3e-6 / 8e-9), and fp32 ARITHMETIC moves it
# chaotically at the 1e-5 ... 1e-4 level: two builds of round 3 that differ only in the ORDER in which the ratings of a
# 64-rating chunk are summed (profiles/r03_ab_gather_row_spread.txt; every other fixture agrees between them to 1e-7)
# gave fold-RMSE errors of 2.0e-6 and 2.4e-5 on the default path (W 7.7e-5 / 1.4e-4 of max, predictions 3.9e-4 / 9.5e-4)
# and 4.5e-5 and 1.5e-4 with the f32-MFMA Gram (W 3.8e-3 / 1.1e-3, predictions 1.2e-2 / 5.4e-3).  Its bands are therefore
# the BUDGET itself on the default path (fold RMSE 1e-4; history, norms and biases stay in the common bands) and a
# documented "outside the 1e-4 budget" for the non-default f32-MFMA Gram mode; float64 mode: 4.3e-7 (TOL64 x 10).
TOL_ILL_POSED = {"g12_wlam0_k80": dict(test_rmse=1e-4, pred=5e-3, f_atol=1e-3)}
# (the f32-MFMA Gram also moves the third-iteration ||V|| by up to 3.4e-6 relative on this fixture: norms 2e-5)
TOL_ILL_POSED_F32_GRAM = {"g12_wlam0_k80": dict(test_rmse=5e-4, pred=5e-2, f_atol=2e-2, f_rtol=0.0, norms=2e-5)}


TOL_ILL_POSED_F64 = {"g12_wlam0_k80": dict(test_rmse=5e-6, pred=1e-3, f_atol=4e-4)}       # observed 4.3e-7 / 7.5e-5 / 2.3e-5


def _tol_for(name, base, gram=None):
    over = TOL_ILL_POSED_F32_GRAM if gram == "f32" else TOL_ILL_POSED_F64 if gram == "f64" else TOL_ILL_POSED
    return dict(base, **over.get(name, {}))


def _close(got, ref, rtol=TOL["f_rtol"], atol_rel=TOL["f_atol"], what=""):
    ref = np.asarray(ref)
    atol = atol_rel * max(float(np.max(np.abs(ref))), 1e-30)
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=what)


def _check_against_fixture(model, g: Golden, tol):
    d = g.d
    ref_h = d["hist_train_rmse"]
    got_h = np.asarray(model.history["train_rmse"])
    assert got_h.shape == ref_h.shape, f"iterations run: {got_h.shape[0]} vs reference {ref_h.shape[0]}"
    assert np.max(np.abs(got_h - ref_h)) <= tol["hist"], np.max(np.abs(got_h - ref_h))
    for key in ("U_norm", "V_norm", "bu_norm", "bi_norm"):
        np.testing.assert_allclose(model.history[key], d["hist_" + key], rtol=tol["norms"], atol=1e-7, err_msg=key)
    if "sel_u" in d.files:
        U, V = model.U[d["sel_u"]], model.V[d["sel_i"]]
    else:
        U, V = model.U, model.V
    _close(U, d["U"], tol["f_rtol"], tol["f_atol"], what="U")
    _close(V, d["V"], tol["f_rtol"], tol["f_atol"], what="V")
    np.testing.assert_allclose(model.b_u, d["b_u"], atol=tol["bias"], rtol=0)
    np.testing.assert_allclose(model.b_i, d["b_i"], atol=tol["bias"], rtol=0)
    assert abs(model.mu - float(d["mu"][0])) <= tol["mu"]
    for f in g.cfg["feats"]:
        _close(model.W[f], d["W_" + f], tol["f_rtol"], tol["f_atol"], what="W_" + f)
    pred = model.predict_at(g.val_flat(), g.features or None)
    np.testing.assert_allclose(pred, d["pred_val"], atol=tol["pred"], rtol=0)
    rmse = float(np.sqrt(np.mean((g.val_truth() - pred) ** 2)))
    assert abs(rmse - float(d["test_rmse"][0])) <= tol["test_rmse"]


@pytest.mark.parametrize("gram", ["f16x2", "f32"])
@pytest.mark.parametrize("name", golden_names())
def test_fit_matches_reference_fixture(name, gram):
    """The DEFAULT path (solve_dtype="auto") in both Gram modes of K1 (2-way fp16 split on the fp16 matrix cores;
    f32 MFMA) is held to the same tight tolerances against the float64 reference on EVERY fixture - including the
    lambda = 1e-2 / 1e-4 corner of the tuner's search space (scripts/tune_params.py:100-101), whose ill-conditioned
    rows the call redoes in fp64, and the rank-deficient lambda_w = 0 designs."""
    _cuda()
    g = Golden(name)
    model = model_for(g, gram=gram)
    r, c, v = g.train
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"],
                  min_iters=g.cfg["min_iters"], verbose=0)
    _check_against_fixture(model, g, _tol_for(name, TOL, gram))


@pytest.mark.parametrize("name", sorted(TOL_FP32_ONLY))
def test_fp32_only_mode_at_small_lambda_is_what_the_docs_say(name):
    """solve_dtype="float32" (no fp64 redo): lambda = 1e-2 stays inside the 1e-4 RMSE budget but outside the tight
    band; lambda = 1e-4 leaves the budget (observed 1e-2) - the fit must still run and stay finite.  This is why
    "auto" is the default."""
    _cuda()
    g = Golden(name)
    model = model_for(g, solve_dtype="float32")
    r, c, v = g.train
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"],
                  min_iters=g.cfg["min_iters"], verbose=0)
    tol = TOL_FP32_ONLY[name]
    if tol is None:
        assert np.all(np.isfinite(model.U)) and np.all(np.isfinite(model.V))
        assert len(model.history["train_rmse"]) == len(g.d["hist_train_rmse"])
        return
    _check_against_fixture(model, g, tol)


@pytest.mark.parametrize("name", golden_names())
def test_fit_float64_matches_reference_fixture(name):
    """solve_dtype="float64" (fp64 Gram / Cholesky / substitutions on fp32-stored factors) is held to the tight
    band on EVERY fixture, including the small-lambda corner where the fp32 solve is outside the 1e-4 budget."""
    _cuda()
    g = Golden(name)
    model = model_for(g, solve_dtype="float64")
    r, c, v = g.train
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"],
                  min_iters=g.cfg["min_iters"], verbose=0)
    _check_against_fixture(model, g, _tol_for(name, TOL64, "f64"))


def test_fit_falls_back_to_level_sweeps_when_the_dataflow_launch_gives_up(monkeypatch):
    """The persistent one-launch sweep raises its error word when a dependency wait exceeds its bound (launch
    not resident as a whole).  `fit` must then refit with the per-level launches and still match the reference."""
    _cuda()
    import collaborative_filtering_amd.als as A
    g = Golden("g5_graph_a0.5")
    r, c, v = g.train
    orig = A._Engine._gs_sweep
    hits = {"n": 0}

    def flaky(self):
        orig(self)
        if self.gs_dataflow and hits["n"] == 0:
            self.gs_err.fill_(1)            # what the kernel does on a timed-out wait
            hits["n"] += 1
    monkeypatch.setattr(A._Engine, "_gs_sweep", flaky)
    monkeypatch.setattr(A, "_DATAFLOW_GAVE_UP", set())      # (the per-device memory of the fallback: restored after the test)
    model = model_for(g)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    assert hits["n"] == 1 and not model._eng.gs_dataflow and not model._dataflow_sweep
    _check_against_fixture(model, g, TOL)
    # the decision is remembered for the device: a NEW model (what a sweep driver makes per fit) starts with the
    # per-level launches instead of paying a failed attempt again
    assert A._DATAFLOW_GAVE_UP
    again = model_for(g).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    assert hits["n"] == 1 and not again._eng.gs_dataflow
    _check_against_fixture(again, g, TOL)


def test_refit_after_a_failed_sweep_leaves_no_history_of_the_failed_run(monkeypatch):
    """Second `fit` of one model (history appends, scripts/als.py:168-176 quirk) whose first attempt at the sweep
    gives up: the failed run must not have appended anything - the history is first fit + the refit, nothing more."""
    _cuda()
    import collaborative_filtering_amd.als as A
    g = Golden("g5_graph_a0.5")
    r, c, v = g.train
    monkeypatch.setattr(A, "_DATAFLOW_GAVE_UP", set())
    model = model_for(g)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    first = list(model.history["train_rmse"])
    orig = A._Engine._gs_sweep
    hits = {"n": 0}

    def flaky(self):
        orig(self)
        if self.gs_dataflow and hits["n"] == 0:
            self.gs_err.fill_(1)
            hits["n"] += 1
    monkeypatch.setattr(A._Engine, "_gs_sweep", flaky)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    assert hits["n"] == 1
    for key in ("train_rmse", "U_norm", "V_norm", "bu_norm", "bi_norm"):
        assert len(model.history[key]) == 2 * len(first), key
    assert model.history["train_rmse"][: len(first)] == first
    # (the refit sweeps level by level: same arithmetic per item, the neighbour sums in another order)
    np.testing.assert_allclose(model.history["train_rmse"][len(first):], first, rtol=0, atol=1e-7)


def test_predict_composes_z_from_the_features_it_is_given():
    """scripts/als.py:568-572: predict builds Z from whatever features are passed.  In-place edits of the fit's
    arrays, or different arrays, must show in the predictions (round 2 short-cut on object identity: stale Z)."""
    _cuda()
    g = Golden("g4_feat_uw1")
    r, c, v = g.train
    feats = {f: np.array(X, copy=True) for f, X in g.features.items()}
    model = model_for(g).fit_coo(r, c, v, (g.m, g.n), features=feats, tol=None, verbose=0)
    idx = g.val_flat()
    base = model.predict_at(idx, feats)
    name = next(iter(feats))
    feats[name] *= 0.5                                      # in place: same object, new contents
    edited = model.predict_at(idx, feats)
    fresh = model.predict_at(idx, {f: np.array(X, copy=True) for f, X in feats.items()})
    np.testing.assert_array_equal(edited, fresh)
    assert np.max(np.abs(edited - base)) > 1e-4
    # expected: U (V + sum_f X_f W_f)^T + mu + b_u + b_i with the edited X
    Z = model.V + sum(np.asarray(feats[f], dtype=np.float64) @ model.W[f] for f in feats)
    u, i = np.divmod(idx, g.n)
    want = np.einsum("tk,tk->t", model.U[u], Z[i]) + model.mu + model.b_u[u] + model.b_i[i]
    np.testing.assert_allclose(edited, want, atol=2e-5, rtol=0)


def test_dense_entry_and_dense_predict():
    """fit(R dense NaN) + predict() -> (m, n) float64, as evaluate_models.py:247-254 uses them."""
    _cuda()
    from tests.synth import to_dense
    g = Golden("g2_bias_pop")
    r, c, v = g.train
    R = to_dense(r, c, v, (g.m, g.n))
    model = model_for(g).fit(R, tol=None, verbose=0)
    R_hat = model.predict()
    assert R_hat.shape == (g.m, g.n) and R_hat.dtype == np.float64
    flat = g.val_flat()
    np.testing.assert_allclose(R_hat.ravel()[flat], g.d["pred_val"], atol=TOL["pred"], rtol=0)
    np.testing.assert_allclose(R_hat.ravel()[flat], model.predict_at(flat), atol=1e-5, rtol=0)


def test_precomputed_graph_entry():
    """fit(..., S=csr) (the GraphSimConfig.source='precomputed' hook) == feature-built graph."""
    _cuda()
    g = Golden("g5_graph_a0.5")
    r, c, v = g.train
    m1 = model_for(g).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    m2 = model_for(g).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0, S=g.S_csr())
    np.testing.assert_allclose(m1.V, m2.V, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(m1.history["train_rmse"], m2.history["train_rmse"], atol=1e-6)


def test_history_appends_on_second_fit():
    _cuda()
    g = Golden("g1_plain")
    r, c, v = g.train
    model = model_for(g)
    model.fit_coo(r, c, v, (g.m, g.n), tol=None, verbose=0)
    model.fit_coo(r, c, v, (g.m, g.n), tol=None, verbose=0)
    assert len(model.history["train_rmse"]) == 2 * g.cfg["n_iters"]      # reference quirk


def test_not_spd_raises_linalgerror():
    _cuda()
    from collaborative_filtering_amd import ALS, ALSConfig, CoreConfig
    g = Golden("g1_plain")
    r, c, v = g.train
    cfg = ALSConfig(core=CoreConfig(n_factors=4, n_iters=2, lambda_u=-50.0, lambda_v=1.0))
    with pytest.raises(np.linalg.LinAlgError):
        ALS(cfg).fit_coo(r, c, v, (g.m, g.n), tol=None, verbose=0)


def test_run_to_run_bitwise_reproducible():
    _cuda()
    g = Golden("g9_k64_mid")
    r, c, v = g.train
    a = model_for(g).fit_coo(r, c, v, (g.m, g.n), tol=None, verbose=0)
    b = model_for(g).fit_coo(r, c, v, (g.m, g.n), tol=None, verbose=0)
    assert np.array_equal(a.U, b.U) and np.array_equal(a.V, b.V)
    assert a.history["train_rmse"] == b.history["train_rmse"]
    # with the Laplacian: the dataflow sweep sums in a timing-independent order
    g = Golden("g5_graph_a0.5")
    r, c, v = g.train
    runs = [model_for(g).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0) for _ in range(3)]
    for other in runs[1:]:
        assert np.array_equal(runs[0].V, other.V) and np.array_equal(runs[0].U, other.U)
        assert runs[0].history["train_rmse"] == other.history["train_rmse"]


@pytest.mark.parametrize("name", ["g5_graph_a0.5", "g5_graph_a5.0"])
def test_graph_without_features_matches_oracle(name):
    """Laplacian on, no feature projections (the benchmark configuration): the statistics come from
    the closed form fused into the sweep (DESIGN.md 'Statistics'); checked against the oracle run on
    the same inputs with the fixture's pinned graph."""
    _cuda()
    from oracle.als_oracle import OracleALS
    g = Golden(name)
    r, c, v = g.train
    cfg = g.oracle_config()
    cfg.lambda_w = {}
    o = OracleALS(cfg).fit(g.train_ratings(), {}, tol=None, S_csr=g.S_csr())
    m = model_for(g)
    m.fit_coo(r, c, v, (g.m, g.n), features=None, tol=None, verbose=0, S=g.S_csr())
    assert m._eng.fused_stats and m._eng.use_graph
    assert np.max(np.abs(np.asarray(m.history["train_rmse"]) - np.asarray(o.history["train_rmse"]))) <= TOL["hist"]
    _close(m.V, o.V, what="V")
    _close(m.U, o.U, what="U")
    assert abs(m.mu - o.mu) <= TOL["hist"]


def test_fused_statistics_equal_the_standalone_pass():
    """Same fit with the fused statistics switched off (standalone als_residual_stats pass)."""
    _cuda()
    g = Golden("g9_k64_mid")
    r, c, v = g.train
    a = model_for(g).fit_coo(r, c, v, (g.m, g.n), tol=None, verbose=0)
    assert a._eng.fused_stats
    import collaborative_filtering_amd.als as A
    orig = A._Engine.stats_step

    def unfused(self, it):
        self.fused_stats = False
        return orig(self, it)
    A._Engine.stats_step = unfused
    try:
        b = model_for(g).fit_coo(r, c, v, (g.m, g.n), tol=None, verbose=0)
    finally:
        A._Engine.stats_step = orig
    np.testing.assert_allclose(a.history["train_rmse"], b.history["train_rmse"], atol=3e-6, rtol=0)
    assert abs(a.mu - b.mu) <= 3e-6


@pytest.mark.parametrize("name", ["g4_feat_uw2", "g4_feat_uw5"])
def test_feature_statistics_closed_form_equals_the_standalone_pass(name):
    """Fits with features: mu / RMSE from the per-item closed form (als_item_stats: item Gram, rhs, column
    sums and the final Z) against the standalone pass over the ratings (als_residual_stats)."""
    _cuda()
    g = Golden(name)
    r, c, v = g.train
    a = model_for(g).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    assert a._eng.fused_feat_stats and not a._eng.fused_stats
    import collaborative_filtering_amd.als as A
    orig = A._Engine.stats_step

    def unfused(self, it):
        self.fused_feat_stats = False
        return orig(self, it)
    A._Engine.stats_step = unfused
    try:
        b = model_for(g).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    finally:
        A._Engine.stats_step = orig
    np.testing.assert_allclose(a.history["train_rmse"], b.history["train_rmse"], atol=3e-6, rtol=0)
    assert abs(a.mu - b.mu) <= 3e-6


def test_cfg2_full_size_against_oracle():
    """BASELINE.json configs[1] at full size (6040 x 3706, 1M ratings, k = 32, explicit bias lambdas):
    three iterations of the HIP path against the oracle on the same seeded input."""
    _cuda()
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
    from oracle.als_oracle import OracleALS, OracleConfig, ratings_from_coo
    from tests.synth import make_ratings
    m, n, k = 6040, 3706, 32
    r, c, v = make_ratings(m, n, 1_000_000, seed=1002)
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=3, lambda_u=5.0, lambda_v=6.0),
                    biases=BiasesConfig(lambda_bu=3.0, lambda_bi=2.0))
    model = ALS(cfg).fit_coo(r, c, v, (m, n), tol=None, verbose=0)
    o = OracleALS(OracleConfig(n_factors=k, n_iters=3, lambda_u=5.0, lambda_v=6.0, lambda_bu=3.0,
                               lambda_bi=2.0)).fit(ratings_from_coo(r, c, v, (m, n)), tol=None)
    assert np.max(np.abs(np.asarray(model.history["train_rmse"]) - np.asarray(o.history["train_rmse"]))) <= TOL["hist"]
    _close(model.U, o.U, what="U")
    _close(model.V, o.V, what="V")
    np.testing.assert_allclose(model.b_u, o.b_u, atol=TOL["bias"], rtol=0)
    np.testing.assert_allclose(model.b_i, o.b_i, atol=TOL["bias"], rtol=0)


def test_features_mid_size_against_oracle():
    """W-step at k = 64 with both features on a 5000 x 1500 / 150K-rating problem (the largest the
    oracle's explicit N_obs x (d k) design matrix allows in a few seconds)."""
    _cuda()
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
    from oracle.als_oracle import OracleALS, OracleConfig, ratings_from_coo
    from tests.synth import make_features, make_ratings
    m, n, k = 5000, 1500, 64
    r, c, v = make_ratings(m, n, 150_000, seed=1003)
    G, Y = make_features(n, 77)
    feats = {"genres": G, "years": Y}
    lw = {"genres": 5.0, "years": 10.0}
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=3, lambda_u=5.0, lambda_v=6.0, update_w_every=2),
                    biases=BiasesConfig(lambda_bu=3.0, lambda_bi=2.0))
    model = ALS(cfg, lambda_w=lw).fit_coo(r, c, v, (m, n), features=feats, tol=None, verbose=0)
    o = OracleALS(OracleConfig(n_factors=k, n_iters=3, lambda_u=5.0, lambda_v=6.0, lambda_bu=3.0, lambda_bi=2.0,
                               update_w_every=2, lambda_w=lw)).fit(ratings_from_coo(r, c, v, (m, n)), feats, tol=None)
    assert np.max(np.abs(np.asarray(model.history["train_rmse"]) - np.asarray(o.history["train_rmse"]))) <= TOL["hist"]
    for f in feats:
        _close(model.W[f], o.W[f], what="W_" + f)
    _close(model.V, o.V, what="V")


@pytest.mark.parametrize("k", [16, 50, 80, 128, 150])
def test_graph_sweep_other_k_against_oracle(k):
    """The dataflow Laplacian sweep for k != 64 (register solve for k <= 64, streamed solve above),
    with a precomputed graph and no features, against the oracle."""
    _cuda()
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig, GraphSimConfig, layout
    from oracle.als_oracle import OracleALS, OracleConfig, ratings_from_coo
    from tests.synth import make_features, make_ratings
    m, n = 400, 300
    r, c, v = make_ratings(m, n, 9000, seed=500 + k)
    G, _ = make_features(n, 9)
    S = layout.build_similarity_dense(G, 8, 1e-8)
    S_csr = layout.dense_graph_to_csr(S)
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=4, lambda_u=3.0, lambda_v=4.0, pop_reg_mode="inverse_sqrt"),
                    biases=BiasesConfig(lambda_bu=2.0, lambda_bi=1.5),
                    graph=GraphConfig(alpha=0.8, sim=GraphSimConfig(source="precomputed")))
    model = ALS(cfg).fit_coo(r, c, v, (m, n), tol=None, verbose=0, S=S_csr)
    assert model._eng.gs_dataflow and model._eng.fused_stats
    o = OracleALS(OracleConfig(n_factors=k, n_iters=4, lambda_u=3.0, lambda_v=4.0, pop_reg_mode="inverse_sqrt",
                               lambda_bu=2.0, lambda_bi=1.5, alpha=0.8, sim={"feature_name": "genres"}))
    o.fit(ratings_from_coo(r, c, v, (m, n)), {}, tol=None,
          S_csr=(S_csr[0], S_csr[1].astype(np.int64), S_csr[2]))
    assert np.max(np.abs(np.asarray(model.history["train_rmse"]) - np.asarray(o.history["train_rmse"]))) <= TOL["hist"]
    _close(model.V, o.V, what="V")
    _close(model.U, o.U, what="U")
    np.testing.assert_allclose(model.b_i, o.b_i, atol=TOL["bias"], rtol=0)


def test_device_graph_build_in_fit():
    """graph_build='device'  gives the same fit as the reference-style host build when the
    graph feature has no ties (continuous embedding)."""
    _cuda()
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig, GraphSimConfig
    from tests.synth import make_ratings
    m, n = 400, 300
    r, c, v = make_ratings(m, n, 9000, seed=77)
    emb = np.random.default_rng(5).normal(size=(n, 6)).astype(np.float32)
    cfg = ALSConfig(core=CoreConfig(n_factors=16, n_iters=4, lambda_u=3.0, lambda_v=4.0),
                    biases=BiasesConfig(2.0, 1.5),
                    graph=GraphConfig(alpha=0.6, sim=GraphSimConfig(feature_name="emb", topk=12)))
    a = ALS(cfg, lambda_w={"emb": 4.0}).fit_coo(r, c, v, (m, n), features={"emb": emb}, tol=None, verbose=0)
    b = ALS(cfg, lambda_w={"emb": 4.0}, graph_build="device").fit_coo(r, c, v, (m, n), features={"emb": emb},
                                                                     tol=None, verbose=0)
    np.testing.assert_allclose(a.history["train_rmse"], b.history["train_rmse"], atol=2e-6, rtol=0)
    np.testing.assert_allclose(a.V, b.V, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", ["g2_bias_pop", "g4_feat_uw2", "g5_graph_a0.5", "g6_early_stop", "g7_k128"])
def test_hip_graph_replay_is_bitwise_the_eager_fit(name):
    """hip_graph=True: iterations after the first are replayed as captured HIP graphs (one per W-step /
    no-W-step variant).  Same launches, same order: every result must be bitwise equal to the eager fit,
    including the early-stopping iteration."""
    _cuda()
    g = Golden(name)
    r, c, v = g.train
    kw = dict(features=g.features or None, tol=g.cfg["tol"], min_iters=g.cfg["min_iters"], verbose=0)
    a = model_for(g).fit_coo(r, c, v, (g.m, g.n), **kw)
    b = model_for(g, hip_graph=True).fit_coo(r, c, v, (g.m, g.n), **kw)
    assert b._eng.graphs_captured > 0                        # also with early stopping (g6: stops at iteration 32)
    assert len(a.history["train_rmse"]) == len(b.history["train_rmse"])
    for key in ("U", "V", "b_u", "b_i"):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key), err_msg=key)
    np.testing.assert_array_equal(a.history["train_rmse"], b.history["train_rmse"])
    assert a.mu == b.mu
    for f in g.cfg["feats"]:
        np.testing.assert_array_equal(a.W[f], b.W[f])


@pytest.mark.parametrize("name,k", [("g5_graph_a0.5", None), ("g10_full_k128", None)])
def test_nondep_prepass_is_bitwise_the_in_sweep_gather(name, k, monkeypatch):
    """The neighbour sums that do not depend on the sweep are formed by a parallel launch before the persistent
    one (k_gs_nondep) with the chunking and summation order of the in-sweep loop: bitwise the same fit."""
    _cuda()
    g = Golden(name)
    r, c, v = g.train
    kw = dict(features=g.features or None, tol=None, verbose=0)
    monkeypatch.setenv("ALS_GS_NONDEP", "1")
    a = model_for(g).fit_coo(r, c, v, (g.m, g.n), **kw)
    assert a._eng.gs_nondep is not None
    monkeypatch.setenv("ALS_GS_NONDEP", "0")
    b = model_for(g).fit_coo(r, c, v, (g.m, g.n), **kw)
    assert b._eng.gs_nondep is None
    np.testing.assert_array_equal(a.V, b.V)
    np.testing.assert_array_equal(a.U, b.U)
    np.testing.assert_array_equal(a.history["train_rmse"], b.history["train_rmse"])


def test_hip_graph_replay_over_many_iterations():
    """30 iterations with features (W-step every 5th) and the Laplacian: the W-step / no-W-step graphs are replayed
    alternately many times (tol=None: no host read-back in between).  Bitwise the eager fit."""
    _cuda()
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig, GraphSimConfig
    g = Golden("g5_graph_a0.5")
    r, c, v = g.train
    cfg = ALSConfig(core=CoreConfig(n_factors=16, n_iters=30, lambda_u=2.0, lambda_v=3.0, pop_reg_mode="inverse_sqrt",
                                    update_w_every=5),
                    biases=BiasesConfig(1.5, 2.5), graph=GraphConfig(alpha=0.5, sim=GraphSimConfig(**g.cfg["sim"])))
    lw = {"genres": 5.0, "years": 10.0}
    a = ALS(cfg, lambda_w=lw).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    b = ALS(cfg, lambda_w=lw, hip_graph=True).fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=None, verbose=0)
    assert b._eng.graphs_captured == 2
    np.testing.assert_array_equal(a.history["train_rmse"], b.history["train_rmse"])
    np.testing.assert_array_equal(a.U, b.U)
    np.testing.assert_array_equal(a.V, b.V)
    for f in lw:
        np.testing.assert_array_equal(a.W[f], b.W[f])


def test_hip_graph_replay_with_early_stopping_reads():
    """Reference-scale shape (610 x 4980, 100K ratings), Laplacian + features (W-step every 5th iteration, so the two
    captured graphs alternate): replay with the per-iteration read-back of early stopping is bitwise the eager fit -
    70 iterations with a tolerance that never triggers, and a fit that does stop early (same stopping iteration).
    Regression test for the memset-node issue (gs_sweep.hip: the publication buffer is reset by a kernel)."""
    _cuda()
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig, GraphSimConfig
    from tests.synth import make_features, make_ratings
    m, n = 610, 4980
    r, c, v = make_ratings(m, n, 100000, 5)
    G, Y = make_features(n, 6)
    feats = {"genres": G, "years": Y}
    lw = {"genres": 31.1, "years": 28.3}
    for n_iters, tol, min_iters in ((70, -1.0, 5), (100, 1e-4, 10)):
        cfg = ALSConfig(core=CoreConfig(n_factors=16, n_iters=n_iters, lambda_u=8.74, lambda_v=7.02,
                                        pop_reg_mode="inverse_sqrt", update_w_every=5),
                        biases=BiasesConfig(3.0, 2.0),
                        graph=GraphConfig(alpha=0.83, sim=GraphSimConfig(feature_name="genres", topk=50, eps=1e-8)))
        a = ALS(cfg, lambda_w=lw).fit_coo(r, c, v, (m, n), features=feats, tol=tol, min_iters=min_iters, verbose=0)
        b = ALS(cfg, lambda_w=lw, hip_graph=True).fit_coo(r, c, v, (m, n), features=feats, tol=tol,
                                                           min_iters=min_iters, verbose=0)
        assert b._eng.graphs_captured == 2
        assert len(a.history["train_rmse"]) == len(b.history["train_rmse"])
        assert (len(a.history["train_rmse"]) == n_iters) == (tol < 0)
        np.testing.assert_array_equal(a.history["train_rmse"], b.history["train_rmse"])
        np.testing.assert_array_equal(a.U, b.U)
        np.testing.assert_array_equal(a.V, b.V)
        for f in lw:
            np.testing.assert_array_equal(a.W[f], b.W[f])


def test_streamed_sweep_form_equals_the_image_form(tmp_path):
    """k > 64 has two forms of the dataflow sweep (factor as an LDS image / streamed during the solve); the
    library picks by the number of items.  The streamed form is forced in a child process (ALS_GS_FORM) and
    must reproduce the image form's fit: same dependency semantics and summation order, only the
    substitution's operand source differs."""
    _cuda()
    import subprocess
    import sys
    script = r'''
import sys, numpy as np
sys.path.insert(0, %r)
from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig, GraphSimConfig, layout
from tests.synth import make_features, make_ratings
k, m, n = 128, 400, 300
r, c, v = make_ratings(m, n, 9000, seed=628)
G, _ = make_features(n, 9)
S_csr = layout.dense_graph_to_csr(layout.build_similarity_dense(G, 8, 1e-8))
cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=4, lambda_u=3.0, lambda_v=4.0, pop_reg_mode="inverse_sqrt"),
                biases=BiasesConfig(lambda_bu=2.0, lambda_bi=1.5),
                graph=GraphConfig(alpha=0.8, sim=GraphSimConfig(source="precomputed")))
model = ALS(cfg).fit_coo(r, c, v, (m, n), tol=None, verbose=0, S=S_csr)
np.savez(sys.argv[1], V=model.V, U=model.U, b_i=model.b_i, rmse=np.asarray(model.history["train_rmse"]))
''' % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))),)
    outs = {}
    for form in ("image", "stream"):
        out = str(tmp_path / f"{form}.npz")
        env = dict(os.environ, ALS_GS_FORM=form)
        res = subprocess.run([sys.executable, "-c", script, out], env=env, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        outs[form] = np.load(out)
    a, b = outs["image"], outs["stream"]
    scale = float(np.abs(a["V"]).max())
    # two fp32 substitution codes on the same factor: agreement well inside the fixture tolerance (2e-4 * max)
    np.testing.assert_allclose(b["V"], a["V"], rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(b["U"], a["U"], rtol=0, atol=1e-4 * float(np.abs(a["U"]).max()))
    np.testing.assert_allclose(b["rmse"], a["rmse"], rtol=0, atol=2e-6)
