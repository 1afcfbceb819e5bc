"""ALS.explain / explain_new and cv.leverage_calibration without a GPU: the C struct mirror and the host logic of the
engine on the numpy stand-in backend, whose `explain` is the contract of als_explain in float64
(`explain_pair` of tests/serving_ref.py; its algebra is checked in tests/test_serving_ref_cpu.py)."""
import os

import numpy as np
import pytest
import torch

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, Explanation, cv
from tests import serving_ref as ref
from tests.cpu_backend import NumpyBackend
from tests.serving_ref import EPS
from tests.synth import make_features, make_ratings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("score", "latent", "leverage", "b_u", "items", "contributions", "weights", "counts")


# ------------------------------------------------------------------------------------------ C ABI
def test_struct_layout_matches_header(tmp_path):
    import ctypes as C
    import subprocess
    from collaborative_filtering_amd import _hip
    st = _hip.ExplainParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "als_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(als_explain_params));']
    src += [f'printf("%zu\\n", offsetof(als_explain_params, {f}));' for f, _ in st._fields_]
    src.append('return 0;}')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = iter(int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(st) == next(vals)
    for f, _ in st._fields_:
        assert getattr(st, f).offset == next(vals), f
    assert "als_explain" in _hip.EXPORTS
    lib = _hip.load()
    assert hasattr(lib, "als_explain") and lib.als_version() == 103


# ------------------------------------------------------------------------------------------ stand-in backend
M_USERS, N_ITEMS, K = 30, 25, 5


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M_USERS, N_ITEMS, 300, seed=3, empty_users=(4,))
    G, y = make_features(N_ITEMS, seed=4)
    feats = {"genres": G, "years": y}
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    be = NumpyBackend()
    model = ALS(cfg, lambda_w={"genres": 1.0, "years": 1.0}, device="cpu", backend=be)
    model.fit_coo(r, c, v, (M_USERS, N_ITEMS), features=feats, tol=None, verbose=0)
    return model, be, feats, r, c, v


def _expected(model, Zfeat, r, c, v, u, i, M, T, largest):
    eng = model._eng
    sel = r == u
    return ref.explain_pair(Zfeat, eng.b_i.numpy(), eng.mu.item(), model.lambda_u, model.lambda_bu,
                            c[sel].astype(np.int32), v[sel].astype(np.float32), K, T, int(i), M, largest)


def _assert_pair(ex, p, e, M):
    cnt = e["items"].size
    assert ex.counts[p] == cnt
    for f in ("score", "latent", "leverage", "b_u"):
        assert getattr(ex, f)[p] == e[f], f
    assert (ex.items[p, :cnt] == e["items"]).all() and (ex.items[p, cnt:] == -1).all()
    assert (ex.contributions[p, :cnt] == e["contributions"]).all() and (ex.contributions[p, cnt:] == 0).all()
    assert (ex.weights[p, :cnt] == e["weights"]).all() and (ex.weights[p, cnt:] == 0).all()


def _user_rows(r, c, v, users):
    ptr = np.zeros(len(users) + 1, np.int64)
    np.cumsum([(r == u).sum() for u in users], out=ptr[1:])
    return ptr, np.concatenate([c[r == u] for u in users]), np.concatenate([v[r == u] for u in users])


def test_pairs_come_back_in_the_order_given(fitted):
    model, be, feats, r, c, v = fitted
    rng = np.random.default_rng(0)
    us = np.concatenate([rng.integers(0, M_USERS, 80), [4, 4, 7, 7, 7]])      # user 4 has no ratings; repeated pairs
    its = np.concatenate([rng.integers(0, N_ITEMS, 80), [0, 24, 3, 3, 3]])
    Z = model._eng.V.numpy()                                                  # no features passed: Z = V
    for M, T, largest in ((3, None, True), (128, 2, False)):
        be.launches.clear()
        ex = model.explain(us, its, M, n_sweeps=T, largest=largest)
        assert len(be.launches) == 1 and be.launches[0][:2] == (np.unique(us).size, us.size)
        for f in FIELDS:
            a = getattr(ex, f)
            assert a.dtype == (np.int64 if f in ("items", "counts") else np.float64), f
            assert a.shape == ((us.size, M) if f in ("items", "contributions", "weights") else (us.size,)), f
        for p, (u, i) in enumerate(zip(us, its)):
            _assert_pair(ex, p, _expected(model, Z, r, c, v, u, i, M, T or 0, largest), M)


def test_chunk_boundary_changes_nothing(fitted, monkeypatch):
    model, be, feats, r, c, v = fitted
    rng = np.random.default_rng(1)
    us, its = rng.integers(0, M_USERS, 70), rng.integers(0, N_ITEMS, 70)
    whole = model.explain(us, its, 4)
    R_new = _user_rows(r, c, v, us)
    whole_new = model.explain_new(R_new, (np.arange(us.size + 1), its), 4)
    monkeypatch.setattr(type(model._eng), "REC_BATCH", 7)
    be.launches.clear()
    parts = model.explain(us, its, 4)
    assert len(be.launches) == -(-np.unique(us).size // 7)
    be.launches.clear()
    parts_new = model.explain_new(R_new, (np.arange(us.size + 1), its), 4)
    assert len(be.launches) == 10
    for f in FIELDS:
        assert np.array_equal(getattr(whole, f), getattr(parts, f)), f
        assert np.array_equal(getattr(whole_new, f), getattr(parts_new, f)), f
        assert np.array_equal(getattr(whole, f), getattr(whole_new, f)), f     # explain == explain_new on the training rows


def test_explain_new_rows_without_targets_and_several_targets(fitted, monkeypatch):
    model, be, feats, r, c, v = fitted
    users = [3, 4, 9, 11, 12]
    tptr = np.array([0, 2, 3, 3, 3, 6])                       # rows 2 and 3 have no targets
    titems = np.array([5, 1, 7, 0, 0, 24])
    monkeypatch.setattr(type(model._eng), "REC_BATCH", 2)     # the chunk of rows (2, 3) has no target: no launch
    be.launches.clear()
    ex = model.explain_new(_user_rows(r, c, v, users), (tptr, titems), 6, features=feats)
    assert [l[:2] for l in be.launches] == [(2, 3), (1, 3)]
    Zf = model._eng._compose_for(feats).numpy()
    for p, (b, i) in enumerate(zip([0, 0, 1, 4, 4, 4], titems)):
        _assert_pair(ex, p, _expected(model, Zf, r, c, v, users[b], i, 6, 0, True), 6)
    # the user without ratings: the empty-row outputs
    eng = model._eng
    assert ex.counts[2] == 0 and ex.latent[2] == 0 and ex.b_u[2] == 0 and (ex.items[2] == -1).all()
    assert ex.score[2] == eng.mu.item() + float(eng.b_i[7])
    z = Zf[7, :K].astype(np.float64)
    assert np.isclose(ex.leverage[2], z @ z / (float(np.float32(model.lambda_u)) + EPS), rtol=1e-13)


def test_features_decide_Z(fitted):
    model, be, feats, r, c, v = fitted
    us, its = np.array([1, 2, 2]), np.array([3, 4, 5])
    be.launches.clear()
    with_f = model.explain(us, its, 5, features=feats)
    without = model.explain(us, its, 5)
    assert torch.equal(be.launches[0][2], model._eng._compose_for(feats))
    assert torch.equal(be.launches[1][2], model._eng.V)
    assert not np.array_equal(with_f.latent, without.latent)
    Zf = model._eng._compose_for(feats).numpy()
    for p in range(3):
        _assert_pair(with_f, p, _expected(model, Zf, r, c, v, us[p], its[p], 5, 0, True), 5)


def test_empty_input(fitted):
    model, be, feats, r, c, v = fitted
    be.launches.clear()
    e1 = model.explain([], np.array([], dtype=np.int64), 7)
    e2 = model.explain_new(np.full((2, N_ITEMS), np.nan), ([0, 0, 0], []), 7)
    e3 = model.explain_new((np.array([0]), np.array([], dtype=np.int64), np.array([])), ([0], []), 7)
    assert not be.launches
    for e in (e1, e2, e3):
        assert isinstance(e, Explanation)
        for f in FIELDS:
            a = getattr(e, f)
            assert a.dtype == (np.int64 if f in ("items", "counts") else np.float64), f
            assert a.shape == ((0, 7) if f in ("items", "contributions", "weights") else (0,)), f


# ------------------------------------------------------------------------------------------ validation
def test_explain_argument_errors(fitted):
    model = fitted[0]
    cfg = ALSConfig(core=CoreConfig(n_factors=3, n_iters=1, lambda_u=1.0, lambda_v=1.0))
    with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
        ALS(cfg, device="cpu", backend=NumpyBackend()).explain([0], [0])
    for M in (0, 129, 2.0, True, None):
        with pytest.raises(ValueError, match="M must be an integer"):
            model.explain([0], [0], M)
        with pytest.raises(ValueError, match="M must be an integer"):
            model.explain_new(np.full((1, N_ITEMS), np.nan), ([0, 1], [0]), M)
    for T in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_sweeps"):
            model.explain([0], [0], n_sweeps=T)
        with pytest.raises(ValueError, match="n_sweeps"):
            model.explain_new(np.full((1, N_ITEMS), np.nan), ([0, 1], [0]), n_sweeps=T)
    for users in ([M_USERS], [-1]):
        with pytest.raises(IndexError, match="user ids"):
            model.explain(users, [0])
    for items in ([N_ITEMS], [-1]):
        with pytest.raises(IndexError, match="item ids"):
            model.explain([0], items)
    with pytest.raises(ValueError):
        model.explain([[0, 1]], [[0, 1]])
    with pytest.raises(ValueError, match="same length"):
        model.explain([0, 1], [0])
    with pytest.raises(ValueError):
        model.explain([0.5], [0])
    with pytest.raises(ValueError, match="rows"):
        model.explain([0], [0], features={"genres": np.zeros((N_ITEMS + 1, 2))})
    with pytest.raises(ValueError, match="infinite"):
        model.explain([0], [0], features={"genres": np.full((N_ITEMS, 2), np.inf)})


def test_explain_new_argument_errors(fitted):
    model = fitted[0]
    R = np.full((2, N_ITEMS), np.nan)
    R[0, 3] = 4.0
    with pytest.raises(ValueError, match="targets must be"):
        model.explain_new(R, [0, 1, 2])
    with pytest.raises(ValueError, match="targets indptr must hold 3 integers"):
        model.explain_new(R, ([0, 1], [0]))
    with pytest.raises(ValueError, match="targets indptr must hold 3 integers"):
        model.explain_new(R, ([0.0, 1.0, 1.0], [0]))
    with pytest.raises(ValueError, match="start at 0"):
        model.explain_new(R, ([0, 2, 1], [0]))
    with pytest.raises(ValueError, match="start at 0"):
        model.explain_new(R, ([1, 1, 1], [0]))
    with pytest.raises(IndexError, match="item ids"):
        model.explain_new(R, ([0, 1, 1], [N_ITEMS]))
    with pytest.raises(ValueError):
        model.explain_new(R, ([0, 1, 1], [0.5]))
    with pytest.raises(ValueError):
        model.explain_new(np.zeros((2, N_ITEMS + 1)), ([0, 1, 1], [0]))
    with pytest.raises(ValueError, match="duplicate"):
        model.explain_new((np.array([0, 2]), np.array([1, 1]), np.array([1.0, 2.0])), ([0, 1], [0]))
    with pytest.raises(ValueError, match="rows"):
        model.explain_new(R, ([0, 1, 1], [0]), features={"genres": np.zeros((N_ITEMS + 1, 2))})


# ------------------------------------------------------------------------------------------ cv
class _StubModel:
    """leverage and prediction are what the test says they are."""

    def __init__(self, n, lev, pred):
        self.V = np.zeros((n, 2))
        self._lev, self._pred = lev, pred
        self.calls = []

    def explain(self, users, items, M=10, *, features=None):
        self.calls.append(("explain", M, features))
        return Explanation(*([None] * 2), np.array([self._lev[(u, i)] for u, i in zip(users, items)], dtype=np.float64),
                           *([None] * 5))

    def predict_at(self, flat_idx, features=None):
        self.calls.append(("predict_at", features))
        n = self.V.shape[0]
        return np.array([self._pred[divmod(int(f), n)] for f in flat_idx], dtype=np.float64)


def test_leverage_calibration_against_a_hand_computed_binning():
    pairs = [(0, 1), (0, 2), (1, 0), (2, 3), (2, 1), (3, 3), (3, 0)]
    lev = dict(zip(pairs, [0.5, 0.1, 0.9, 0.3, 0.3, 0.7, 0.2]))
    vals = np.array([4.0, 3.0, 5.0, 2.0, 1.0, 3.5, 4.5])
    err = np.array([1.0, 0.0, -2.0, 0.5, 3.0, -1.0, 2.0])
    pred = {p: x + e for p, x, e in zip(pairs, vals, err)}
    stub = _StubModel(4, lev, pred)
    rows, cols = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    feats = {"genres": np.zeros((4, 1))}
    out = cv.leverage_calibration(stub, rows, cols, vals, features=feats, n_bins=3)
    # sorted by leverage (stable): 0.1 (e 0), 0.2 (e 2), 0.3 (e .5), 0.3 (e 3), 0.5 (e 1), 0.7 (e -1), 0.9 (e -2);
    # 7 pairs in 3 groups: 3, 2, 2
    assert out["count"] == [3, 2, 2]
    np.testing.assert_allclose(out["leverage"], [0.2, 0.4, 0.8], rtol=1e-15)
    np.testing.assert_allclose(out["rmse"], [np.sqrt((0 + 4 + 0.25) / 3), np.sqrt((9 + 1) / 2), np.sqrt((1 + 4) / 2)],
                               rtol=1e-15)
    assert stub.calls == [("explain", 1, feats), ("predict_at", feats)]
    out = cv.leverage_calibration(stub, rows[:2], cols[:2], vals[:2], n_bins=3)         # more bins than pairs
    assert out["count"] == [1, 1, 0] and np.isnan(out["rmse"][2]) and np.isnan(out["leverage"][2])
    np.testing.assert_allclose(out["rmse"][:2], [0.0, 1.0])
    with pytest.raises(ValueError, match="same length"):
        cv.leverage_calibration(stub, rows, cols, vals[:-1])
    with pytest.raises(ValueError, match="n_bins"):
        cv.leverage_calibration(stub, rows, cols, vals, n_bins=0)


def test_leverage_calibration_through_the_model(fitted):
    model, be, feats, r, c, v = fitted
    rng = np.random.default_rng(5)
    rows, cols = rng.integers(0, M_USERS, 40), rng.integers(0, N_ITEMS, 40)
    vals = rng.integers(1, 11, 40) * 0.5
    out = cv.leverage_calibration(model, rows, cols, vals, features=feats, n_bins=4)
    lev = model.explain(rows, cols, 1, features=feats).leverage
    pred = model.predict_at(rows * N_ITEMS + cols, features=feats)
    order = np.argsort(lev, kind="stable")
    assert out["count"] == [10, 10, 10, 10]
    for b in range(4):
        g = order[10 * b: 10 * b + 10]
        assert out["leverage"][b] == lev[g].mean()
        assert out["rmse"][b] == np.sqrt(((pred[g] - vals[g]) ** 2).mean())
    assert out["leverage"] == sorted(out["leverage"])
