"""`ImplicitALS` - the confidence-weighted fit for implicit feedback (Hu, Koren, Volinsky, ICDM 2008) behind the
serving surface of `ALS`.

Ratings r_ui > 0 on the observed pairs (click, play, purchase counts).  With

    a_ui = alpha r_ui  ("linear")   or   alpha log1p(r_ui / eps)  ("log"),      t_ui = 1 + a_ui,

the objective is

    a0 sum_all (u.v)^2 + sum_obs [a (u.v)^2 - 2 t (u.v) + t] + lambda_u |U|^2 + lambda_v |V|^2,

for a0 = 1 exactly the paper's sum_all c (p - u.v)^2 with preference p = 1 and confidence c = 1 + a on the observed
pairs, p = 0 and c = 1 elsewhere.  A half-step solves per row (F the other side's table)

    (a0 F^T F + sum_t a_t f_t f_t^T + (lambda + 1e-10) I) x = sum_t t_t f_t

in fp64 (als_table_gram_f64 once per half-step, als_implicit_row_solve per row).  `item_weight` / `user_weight` put
rank-one weights p_u q_i on the all-entries term, a0 sum_all p_u q_i (u.v)^2 (section 33): a user row then takes
(a0 p_u) sum_i q_i v_i v_i^T, an item row (a0 q_i) sum_u p_u u_u u_u^T - still one Gram per half-step.
There are no biases, no mu, no
features and no graph: predict is U V^T, and everything `serving._Serving` offers on `U V Z b_u b_i mu csr` works
on the fitted tables with b_u = b_i = 0, mu = 0, Z = V.

This module holds `ImplicitConfig`, the fit engine `_ImplicitEngine` and the facade `ImplicitALS`.
"""
from __future__ import annotations

import functools
import inspect
import logging
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import layout
from .als import ALS, _on
from .als_config import ALSConfig
from .containers import _SideDev, _side_to_dev, _tasks_to_dev
from .engine import SCALE_FACTOR, _Engine
from .serving import _Serving, _raise_unless_solved

logger = logging.getLogger(__name__)

CONFIDENCES = ("linear", "log")
ITEM_WEIGHTS = ("popularity",)
DIAG_EPS = 1e-10        # what als_implicit_row_solve adds to lambda on the diagonal (as every row solve here does)


@dataclass
class ImplicitConfig:
    alpha: float = 40.0                 # confidence gain: a = alpha r ("linear") or alpha log1p(r / eps) ("log")
    confidence: str = "linear"
    eps: float = 1.0                    # scale of the counts under "log"
    unobserved_weight: float = 1.0      # a0, the weight of (u.v)^2 on every entry of the matrix
    # rank-one weights p_u q_i on that all-entries term; None: 1 for every user / item
    item_weight: object = None          # "popularity", or an array [n], finite and >= 0
    popularity_exponent: float = 0.5    # eta of "popularity": q_i proportional to (entries of item i) ** eta
    user_weight: object = None          # an array [m], finite and >= 0


def popularity_weights(counts, exponent: float) -> np.ndarray:
    """q (float32 [n]) of `item_weight="popularity"`: q_i = n f_i^eta / sum_j f_j^eta for the entry counts f, evaluated
    in float64 and rounded once, so that the mean is 1 and a0 keeps its meaning.  0^0 = 1 (eta = 0 is uniform); without
    any entry q = 1."""
    f = np.asarray(counts, dtype=np.float64)
    w = f ** float(exponent)
    total = w.sum()
    if not total > 0:
        return np.ones(f.size, dtype=np.float32)
    return ((f.size * w) / total).astype(np.float32)


def _weight_array(x, length: int, name: str) -> np.ndarray:
    """A user's `user_weight` / `item_weight` array as the device stores it (float32 [length]), or ValueError."""
    w = np.asarray(x, dtype=np.float64)
    if w.ndim != 1 or w.size != length:
        raise ValueError(f"ImplicitConfig.{name} must have one value per row ({length}), got shape {w.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        w32 = w.astype(np.float32)
    if w.size and not bool((np.isfinite(w32) & (w32 >= 0)).all()):
        raise ValueError(f"ImplicitConfig.{name} must be finite and >= 0")
    return w32


def confidence_weights(vals, cfg: ImplicitConfig):
    """a (float32) of the ratings `vals` (numpy array or torch tensor), evaluated in float64 and rounded once."""
    if torch.is_tensor(vals):
        r = vals.to(torch.float64)
        a = cfg.alpha * (r if cfg.confidence == "linear" else torch.log1p(r / cfg.eps))
        return a.to(torch.float32)
    r = np.asarray(vals, dtype=np.float64)
    a = cfg.alpha * (r if cfg.confidence == "linear" else np.log1p(r / cfg.eps))
    return a.astype(np.float32)


def check_ratings(vals) -> None:
    """Implicit ratings are positive finite counts; anything else has no confidence."""
    v = vals if torch.is_tensor(vals) else torch.from_numpy(np.ascontiguousarray(vals))
    if v.numel() and not bool((torch.isfinite(v) & (v > 0)).all()):
        raise ValueError("implicit ratings must be finite and > 0 (an unobserved pair is simply absent)")


class _ImplicitEngine(_Serving):
    """Device state and the iteration loop of one `ImplicitALS.fit`; what reads the fitted state afterwards is
    inherited from serving._Serving."""

    def __init__(self, model, csr, csc, device, backend):
        import weakref
        self.model = weakref.proxy(model)           # (no reference cycle with the model: see engine._Engine)
        self.dev, self.be = device, backend
        self.world, self.rank = 1, 0
        self.native = getattr(backend, "lib", None) is not None
        self._init_shapes(model, csr, csc)
        self._init_missing_weights(model, csc)
        self._init_sides(model, csr, csc)
        self._init_tasks()
        self._init_params(model)
        self._init_scratch(model)

    # -------------------------------------------------- construction stages
    def _init_shapes(self, model, csr, csc):
        k = int(model.n_factors)
        self.k, self.ld = k, layout.padded_k(k)
        self.m, self.n = csr.nrows, csc.nrows
        self.nnz = int(csr.vals.shape[0])
        self.a0 = float(model.implicit.unobserved_weight)
        self.feat_names, self.feat_dims = [], []

    def _init_missing_weights(self, model, csc):
        """p (fp32 [m]) and q (fp32 [n]) of the all-entries term a0 sum_all p_u q_i (u.v)^2 on the device, or None
        where the model has none (every value 1).  The same rounded values feed the Gram and the per-row scale."""
        ic = model.implicit
        self.p = self.q = None
        if ic.user_weight is not None:
            self.p = torch.from_numpy(_weight_array(ic.user_weight, self.m, "user_weight")).to(self.dev)
        if isinstance(ic.item_weight, str):
            ptr = csc.indptr.cpu().numpy() if torch.is_tensor(csc.indptr) else np.asarray(csc.indptr)
            counts = np.diff(ptr.astype(np.int64))
            self.q = torch.from_numpy(popularity_weights(counts, ic.popularity_exponent)).to(self.dev)
        elif ic.item_weight is not None:
            self.q = torch.from_numpy(_weight_array(ic.item_weight, self.n, "item_weight")).to(self.dev)

    def _init_sides(self, model, csr, csc):
        """The ratings in HBM with the confidence weights a IN PLACE of the values: the kernels read nothing else per
        rating, and t = 1 + a is formed on the fly."""
        def weighted(s):
            return _side_to_dev(type(s)(s.nrows, s.ncols, s.indptr, s.indices,
                                        confidence_weights(s.vals, model.implicit)), self.dev)
        self.csr, self.csc = weighted(csr), weighted(csc)
        # sum_obs t = nnz + sum a: the constant of the closed-form loss
        self.sum_t = float(self.nnz + self.csr.vals.to(torch.float64).sum().item())

    def _row_tasks(self, ptr: np.ndarray):
        """Task list of all rows of one orientation; no dual-form classes (this kernel has one form)."""
        if self.native:
            t = layout.build_row_tasks_native(self.be.lib, ptr, 0, ptr.size - 1, dual_len=0, mid_len=0)
        else:
            t = layout.build_row_tasks(ptr, 0, ptr.size - 1, dual_len=0, mid_len=0)
        return _tasks_to_dev(t, self.dev)

    def _init_tasks(self):
        self.utasks = self._row_tasks(self.csr.indptr.cpu().numpy())
        self.itasks = self._row_tasks(self.csc.indptr.cpu().numpy())

    def _init_params(self, model):
        # initial factors: the draws of engine._Engine (U first, then V), storage [rows + 1, ld] with a zero last row
        k, f32, f64 = self.k, torch.float32, torch.float64
        rng = np.random.default_rng(model.random_state)

        def padded(A64):
            out = np.zeros((A64.shape[0] + 1, self.ld), dtype=np.float32)
            out[: A64.shape[0], :k] = A64
            return torch.from_numpy(out).to(self.dev)
        self.U_store = padded(rng.normal(scale=SCALE_FACTOR, size=(self.m, k)))
        self.V_store = padded(rng.normal(scale=SCALE_FACTOR, size=(self.n, k)))
        self.U, self.V = self.U_store[: self.m], self.V_store[: self.n]
        self.Z = self.V
        self.b_u = torch.zeros(self.m, dtype=f32, device=self.dev)
        self.b_i = torch.zeros(self.n, dtype=f32, device=self.dev)
        self.mu = torch.zeros(1, dtype=f64, device=self.dev)
        self.W64 = {}

    def _init_scratch(self, model):
        f64 = torch.float64
        ng = self.ld // 16 * (self.ld // 16 + 1) // 2 * 256
        self.G = torch.zeros(ng, dtype=f64, device=self.dev)            # a Gram image (als_table_gram_f64)
        self.G_fold = None                                              # F^T F of the FITTED V, for fold-in calls
        self.xb = torch.zeros(max(self.n, 1), dtype=f64, device=self.dev)
        self.ss = torch.zeros(2, dtype=f64, device=self.dev)            # |U|^2, |V|^2
        self.status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.hist = torch.zeros(max(int(model.n_iters), 1), dtype=f64, device=self.dev)
        self.timers = None
        self.iters_run = 0

    # ---------------------------------------------------------- half steps
    _tick = _Engine._tick           # (name, start, end) events per phase when self.timers is a list

    def _half_step(self, name, side, tasks, F_store, nF, lam, X_out, xb_out, w_table=None, w_rows=None):
        """w_table: the weights of the rows of F in the Gram; w_rows: the per-row scale of that Gram.  Either keyword
        reaches the backend only when its weights are set: an unweighted model makes the calls it always made."""
        gram_kw = {} if w_table is None else {"w": w_table}
        solve_kw = {} if w_rows is None else {"g_scale_row": w_rows}
        with self._tick("table_gram"):
            self.be.table_gram(self.k, self.ld, F_store[:nF], self.G, **gram_kw)
        with self._tick(name):
            self.be.implicit_row_solve(k=self.k, ld=self.ld, side=side, F=F_store, zero_row=nF, G=self.G,
                                       g_scale=self.a0, lam=lam, lam_row=None, X_out=X_out, xb_out=xb_out,
                                       status=self.status, tasks=tasks, **solve_kw)

    def user_step(self):
        self._half_step("row_solve_user", self.csr, self.utasks, self.V_store, self.n, self.model.lambda_u, self.U,
                        None, self.q, self.p)

    def item_step(self):
        self._half_step("row_solve_item", self.csc, self.itasks, self.U_store, self.m, self.model.lambda_v, self.V,
                        self.xb, self.p, self.q)

    def loss_step(self, it):
        """Because A x = b for every item row after the V-step, the G, weighted and lambda_v terms of the loss add up to
        sum_i x_i.b_i - 1e-10 |V|^2 (A carries lambda_v + 1e-10 on its diagonal), so the loss is
        sum_obs t - sum_i x_i.b_i - 1e-10 |V|^2 + lambda_u |U|^2: no pass over the ratings."""
        self.be.sumsq(self.U, self.ss[0:1])
        self.be.sumsq(self.V, self.ss[1:2])
        self.hist[it] = (self.sum_t - self.xb[: self.n].sum() - DIAG_EPS * self.ss[1]
                         + float(self.model.lambda_u) * self.ss[0])

    def iteration(self, it: int, n_iters: Optional[int] = None):
        """One iteration, asynchronous on the stream: Gram(V), U-step, Gram(U), V-step, loss."""
        self.G_fold = None
        self.user_step()
        self.item_step()
        self.loss_step(it)
        self.iters_run = it + 1

    def _check_status(self):
        bad = int(self.status.item())
        if bad:
            self.status.zero_()
            raise np.linalg.LinAlgError(f"normal equations of row {bad - 1} are not positive definite")

    def run(self, tol, min_iters, verbose):
        seen = []
        for it in range(int(self.model.n_iters)):
            self.iteration(it)
            if tol is not None:
                seen.append(float(self.hist[it].item()))
                if it + 1 >= min_iters:
                    self._check_status()
                    # the rule engine._Engine.run applies to the train RMSE, on the relative decrease of the loss
                    if len(seen) >= 3 and seen[-3] - seen[-1] <= tol * abs(seen[-3]):
                        if verbose > 0:
                            logger.info("Early stopping at iter %d; relative loss decrease <= %.3g", it + 1, tol)
                        break
        self._check_status()

    def export(self, model):
        k = self.k
        model.U = self.U[:, :k].to(torch.float64).cpu().numpy()
        model.V = self.V[:, :k].to(torch.float64).cpu().numpy()
        model.b_u = np.zeros(self.m, dtype=np.float64)
        model.b_i = np.zeros(self.n, dtype=np.float64)
        model.mu = 0.0
        model.history["loss"].extend(float(x) for x in self.hist[: self.iters_run].cpu().numpy())

    # -------------------------------------------------- users outside the fit
    def _fold_in_dev(self, indptr: np.ndarray, indices: np.ndarray, vals: np.ndarray, Z, n_sweeps: int):
        """A new user's row is one implicit row solve against the fitted item table: folded factors (fp32 [B, ld]) and
        zero biases on the device, with the device CSR they were computed from.  `n_sweeps` is accepted and ignored:
        there is no bias recurrence.  A new user has p = 1; the Gram is G_q = sum_i q_i z_i z_i^T of the fit's item
        weights (the cached image is that weighted Gram)."""
        md = self.model
        check_ratings(vals)
        B = indptr.size - 1
        ptr_d, idx_d, a_d = self._csr_dev(indptr, indices, confidence_weights(vals, md.implicit))
        if self.G_fold is None or self.G_fold[0] != Z.data_ptr():
            G = torch.zeros_like(self.G)
            self.be.table_gram(self.k, self.ld, Z, G, **({} if self.q is None else {"w": self.q}))
            self.G_fold = (Z.data_ptr(), G)
        U = torch.empty(B, self.ld, dtype=torch.float32, device=self.dev)
        b = torch.zeros(B, dtype=torch.float32, device=self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.be.implicit_row_solve(k=self.k, ld=self.ld, side=_SideDev(B, self.n, ptr_d, idx_d, a_d), F=Z, zero_row=-1,
                                   G=self.G_fold[1], g_scale=self.a0, lam=md.lambda_u, lam_row=None, X_out=U,
                                   xb_out=None, status=status, tasks=self._row_tasks(np.asarray(indptr, np.int64)))
        _raise_unless_solved(status, "fold-in")
        return U, b, ptr_d, idx_d


# calls defined on the explicit row system Z_S^T Z_S + lambda I; an implicit row's system includes G
_UNDEFINED = ("explain", "explain_new", "recommend_explore", "recommend_new_explore", "fold_in_items",
              "predict_new_items")


class ImplicitALS(ALS):
    """Confidence-weighted ALS for implicit feedback: R_hat = U V^T.  `fit`, `fit_coo`, `fit_csr` and the serving
    calls are `ALS`'s; uses n_factors, n_iters, lambda_u, lambda_v and random_state of `config.core`."""

    def __init__(self, config: ALSConfig, implicit: Optional[ImplicitConfig] = None, *, device=None, backend=None,
                 lambda_w=None, process_group=None) -> None:
        super().__init__(config, device=device, backend=backend)
        self.implicit = implicit if implicit is not None else ImplicitConfig()
        ic = self.implicit
        if lambda_w:
            raise ValueError("ImplicitALS has no feature projections: lambda_w is not accepted")
        if process_group is not None:
            raise ValueError("ImplicitALS fits on one device: process_group is not accepted")
        if self.pop_reg_mode:
            raise ValueError("ImplicitALS has no popularity-scaled regularisation: pop_reg_mode must be None")
        if self.alpha > 0.0 and self.cfg.graph.sim is not None:
            raise ValueError("ImplicitALS has no graph regularisation: graph.alpha must be 0 or graph.sim None")
        if ic.confidence not in CONFIDENCES:
            raise ValueError(f"unknown confidence '{ic.confidence}': one of {CONFIDENCES}")
        if not (np.isfinite(ic.alpha) and ic.alpha >= 0):
            raise ValueError("ImplicitConfig.alpha must be >= 0")
        if not (np.isfinite(ic.eps) and ic.eps > 0):
            raise ValueError("ImplicitConfig.eps must be > 0")
        if not (np.isfinite(ic.unobserved_weight) and ic.unobserved_weight >= 0):
            raise ValueError("ImplicitConfig.unobserved_weight must be >= 0")
        if isinstance(ic.item_weight, str) and ic.item_weight not in ITEM_WEIGHTS:
            raise ValueError(f"unknown item_weight '{ic.item_weight}': one of {ITEM_WEIGHTS}, or an array")
        if not (np.isfinite(ic.popularity_exponent) and ic.popularity_exponent >= 0):
            raise ValueError("ImplicitConfig.popularity_exponent must be finite and >= 0")
        self.history["loss"] = []

    def missing_weights(self):
        """(p [m], q [n]) as float32 numpy arrays: the weights p_u q_i the last fit put on the all-entries term, ones
        where `user_weight` / `item_weight` is unset."""
        eng = self._eng
        if eng is None:
            raise RuntimeError("missing_weights() needs a fitted model")
        p = np.ones(eng.m, dtype=np.float32) if eng.p is None else eng.p.cpu().numpy().copy()
        q = np.ones(eng.n, dtype=np.float32) if eng.q is None else eng.q.cpu().numpy().copy()
        return p, q

    def _fit_sides(self, csr, csc, features, tol, min_iters, verbose, S, run: bool = True,
                   S_trusted: bool = False) -> "ImplicitALS":
        if features:
            raise ValueError("ImplicitALS takes no features")
        if S is not None:
            raise ValueError("ImplicitALS takes no similarity graph")
        check_ratings(csr.vals)
        device = self._device or torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        backend = self._backend
        if backend is None:
            from .backend import HipBackend
            backend = HipBackend(device)
        with _on(device):
            self._eng = _ImplicitEngine(self, csr, csc, device, backend)
            if not run:
                return self
            self._eng.run(tol, min_iters, verbose)
            self._eng.export(self)
        if verbose > 0 and self.history["loss"]:
            logger.info("Implicit ALS training finished. Final loss: %.6g", self.history["loss"][-1])
        return self


def _guard(name):
    """The one place that refuses what this model does not define: the calls of `_UNDEFINED`, and `new_items=` (folded
    items come from `fold_in_items`) on every call that takes it."""
    base = getattr(ALS, name)

    @functools.wraps(base)
    def call(self, *args, **kw):
        if name in _UNDEFINED:
            raise ValueError(f"{name} is not defined for ImplicitALS: it is built on the explicit row system "
                             "Z_S^T Z_S + lambda I, an implicit row's system includes the all-entries Gram")
        if kw.get("new_items") is not None:
            raise ValueError(f"{name}(new_items=...) is not defined for ImplicitALS: there is no item fold-in")
        return base(self, *args, **kw)
    return call


for _name, _fn in list(vars(ALS).items()):
    if (inspect.isfunction(_fn) and not _name.startswith("_")
            and (_name in _UNDEFINED or "new_items" in inspect.signature(_fn).parameters)):
        setattr(ImplicitALS, _name, _guard(_name))
