"""The fit engine behind `ALS.fit` (als.py constructs one `_Engine` per fit; nothing here imports als.py).

Every engine attribute exists after construction - `None` (flags: `False`) where it does not apply - and what the
backend can do is read once (`_decide_paths`): the step methods branch on those booleans only.  The containers the
state is made of are containers.py; what reads the fitted state afterwards is serving._Serving."""
from __future__ import annotations

import contextlib
import logging
import os

import numpy as np
import torch
import torch.distributed as dist

from . import layout
from .containers import FitCache, _RowShift, _side_to_dev, _tasks_to_dev, _to_dev
from .serving import _Serving, concat_features
from .validate import _validate_graph

SCALE_FACTOR = 0.1      # scripts/als.py:93
EPS = 1e-10             # scripts/als.py:94
W_F64_BELOW = 1e-2      # solve_dtype="auto": fp64 V-step by-products when some lambda_w (+ 1e-10) is below this

logger = logging.getLogger(__name__)


class SweepNotResident(RuntimeError):
    """The persistent one-launch form of the Laplacian sweep (als_gs_sweep_dataflow) found some of its waves not
    running - another kernel or process held compute units - and gave up; `ALS.fit` then refits with the
    per-level launches, which have no residency requirement."""


class _Engine(_Serving):
    """Device state and the iteration loop of one `fit`: construction (uploads, sharding, task lists, level
    schedule), the half steps, the sweep, the W-step, the statistics, and iteration / replay / run / export.
    What reads the fitted state afterwards is inherited from serving._Serving."""

    U_CHUNKS = 2        # sub-ranges of a rank's user shard (multi-rank runs only; ALS_U_CHUNKS overrides)

    def __init__(self, model, csr, csc, features, S_csr, device, backend, pg, gs_mode, dataflow=True):
        import weakref
        # no reference cycle with the model (which owns this engine): both then die by reference count, at a
        # deterministic point - a cyclic-GC pass destroying captured HIP graphs in the middle of ANOTHER engine's
        # stream capture is an error ("operation not permitted when stream is capturing")
        self.model = weakref.proxy(model)
        self.dev, self.be = device, backend
        self._init_group(pg)
        self._init_shapes(model, csr, csc, features)
        self._decide_paths(model, S_csr, gs_mode, dataflow)
        cache = model._fit_cache if model._fit_cache is not None else FitCache()     # (else: for this fit alone)
        ku, ki = cache.pin(csr), cache.pin(csc)
        init_key, init_future = self._start_init_draw(model, cache)
        counts = self._init_shards(cache, csr, csc, ku, ki)
        self._init_params(model, cache, ku, init_key, init_future)
        self._init_features(cache, features)
        self._init_item_reg(model, counts)
        self._init_graph(model, cache, S_csr, ki, counts > 0)
        self._init_byproducts()
        self._init_wstep()
        self._init_scratch(model)

    # -------------------------------------------------- construction stages
    def _init_group(self, pg):
        # sharding is opt-in: process_group="world" (the default group) or a ProcessGroup object; None fits on
        # this rank alone even when torch.distributed happens to be initialised
        if isinstance(pg, str):
            if pg != "world":
                raise ValueError("process_group must be None, 'world' or a torch.distributed ProcessGroup")
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError("process_group='world' needs an initialised torch.distributed")
            self.pg, self.dist_on = None, True
        else:
            self.pg, self.dist_on = pg, pg is not None
        if self.dist_on:
            self.world, self.rank = dist.get_world_size(self.pg), dist.get_rank(self.pg)
        else:
            self.world, self.rank = 1, 0
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                logger.info("torch.distributed is initialised (world %d) but no process_group was given: "
                            "fitting on this rank alone", dist.get_world_size())
        # `multi`: take the sharded code path with its collectives.  ALS_FORCE_COLLECTIVES=1 takes it on a
        # one-rank group too, to rehearse the RCCL calls on a single GPU (bench.py / tests only).
        self.multi = self.world > 1 or (os.environ.get("ALS_FORCE_COLLECTIVES") == "1" and self.dist_on)

    def _init_shapes(self, model, csr, csc, features):
        k = int(model.n_factors)
        self.k, self.ld = k, layout.padded_k(k)
        self.m, self.n = csr.nrows, csc.nrows
        self.nnz = int(csr.vals.shape[0])
        self.timers = None              # set to [] to record (name, start, end) events per phase
        self.perm = torch.from_numpy(layout.perm_of_col(k)).to(self.dev)     # storage col -> perm pos
        self.feat_names = list(features)
        self.feat_dims = [int(features[f].shape[1]) for f in self.feat_names]

    def _decide_paths(self, model, S_csr, gs_mode, dataflow):
        """What the backend can do, read once, and every choice of path that follows from it.  The backend is duck
        typed on purpose (the numpy stand-in of the CPU tests lacks some entries); nothing after this asks it."""
        be = self.be
        self.native = getattr(be, "lib", None) is not None   # HIP backend: set-up passes in the library too
        self.has_gs_levels = hasattr(be, "gs_levels")                                     # (csrc/host_setup.cpp)
        self.has_history_row = hasattr(be, "history_row")
        self.has_item_stats = hasattr(be, "item_stats")
        has_sum_pairs = hasattr(be, "sum_pairs")
        # The V-step in fp64 with fp64 by-products (item Grams, right-hand sides, Cholesky factors, column sums) for
        # the W-step / the sweep / the item statistics: always under solve_dtype="float64"; under "auto" / "refine" when a
        # feature's ridge parameter is (nearly) absent - lambda_w missing means 0 (scripts/als.py:497) - because the
        # (d k)^2 system is then singular up to the 1e-10 the reference adds and normal equations assembled from
        # fp32 Grams (rounding ~3e-7 |A|) are no longer positive definite, let alone accurate.
        lw_min = min((float(model.lambda_w.get(f, 0.0)) for f in self.feat_names), default=float("inf"))
        mode = getattr(be, "solve_dtype", "float32")
        self.v_f64 = bool(self.native and (mode == "float64" or (mode in ("auto", "refine") and lw_min + EPS < W_F64_BELOW)))
        self.f64kw = {"f64": True} if self.v_f64 else {}        # what the V-step-side backend calls are given then
        self.use_graph = S_csr is not None
        # Sweep modes with several ranks (one rank: all the same thing):
        #   "exact"  (default) the item shards sweep ONE AFTER THE OTHER in rank order, each followed by a
        #            broadcast of its rows: shard r sees the new rows of shards < r and the old rows of
        #            shards > r - the reference's Gauss-Seidel order, at the cost of a sweep that does not
        #            scale with the number of ranks;
        #   "block"  all shards sweep at once, rows of other shards are the previous iteration's
        #            (Gauss-Seidel inside a shard, Jacobi across shards: approximate, scales);
        #   "levels" global level schedule with an exchange after every level (exact; one collective per level).
        self.gs_mode = (gs_mode or "exact") if self.use_graph else None
        if self.use_graph and self.gs_mode not in ("exact", "block", "levels"):
            raise ValueError(f"unknown gs_mode '{self.gs_mode}'")
        # persistent dataflow sweep (one launch, no level barriers) when the backend has it
        self.gs_dataflow = bool(self.use_graph and hasattr(be, "gs_dataflow") and dataflow and not self.v_f64
                                and not (self.multi and self.gs_mode == "levels"))
        # --- fused statistics (DESIGN.md "Statistics"): without features Z == V, so the residual
        #     sums of an iteration follow in closed form from what the V-step already holds
        self.fused_stats = ((not self.feat_names) and has_sum_pairs
                            and (self.ld <= 64 or not self.use_graph or self.gs_dataflow or self.v_f64))
        # with features Z != V: the same sums follow per item from the V-step's Gram / rhs / column sums
        # and the final Z (als_item_stats), again without a pass over the ratings
        self.fused_feat_stats = bool(self.feat_names) and self.has_item_stats and has_sum_pairs

    def _start_init_draw(self, model, cache):
        """--- initial factors (scripts/als.py:329,360-376): numpy's Generator on the host, same seed and draw order
        as the reference.  At 1M x 64 that is 0.8 s of Generator.normal (the reference pays the same); it runs in
        a worker thread (numpy releases the GIL) underneath the rest of the set-up.  Returns (cache key, future or
        None when the cache already holds the draw)."""
        k = self.k
        init_key = ("init", model.random_state, self.m, self.n, k, tuple(self.feat_dims))

        def draw_init_host():
            rng = np.random.default_rng(model.random_state)
            U0 = self._padded_host(rng.normal(scale=SCALE_FACTOR, size=(self.m, k)))
            V0 = self._padded_host(rng.normal(scale=SCALE_FACTOR, size=(self.n, k)))
            W0 = [rng.normal(scale=SCALE_FACTOR, size=(d, k)) for d in self.feat_dims]
            return U0, V0, W0

        if cache.has(init_key):
            return init_key, None
        import concurrent.futures
        pool = concurrent.futures.ThreadPoolExecutor(max_workers=1)
        init_future = pool.submit(draw_init_host)
        pool.shutdown(wait=False)
        return init_key, init_future

    def _tasks_dev(self, cache, key_side, ptr, lo, hi):
        dl = layout.dual_max_len(self.k)          # rows this short are solved in the dual form (k_row_dual)
        dm = layout.dual_mid_len(self.k)          # ... and rows up to this length above k = 96 (k_row_dual_mid)

        def build():
            if self.native:
                return layout.build_row_tasks_native(self.be.lib, ptr, lo, hi, dual_len=dl, mid_len=dm)
            return layout.build_row_tasks(ptr, lo, hi, dual_len=dl, mid_len=dm)
        return cache.get(("tasks", key_side, lo, hi, dl, dm), lambda: _tasks_to_dev(build(), self.dev))

    def _init_shards(self, cache, csr, csc, ku, ki):
        """Ratings upload, shards, task lists, workspace and the control block; returns the ratings per item."""
        # --- ratings in HBM
        self.csr = cache.get(("side_dev", ku), lambda: _side_to_dev(csr, self.dev))
        self.csc = cache.get(("side_dev", ki), lambda: _side_to_dev(csc, self.dev))
        # scale of the fp16 residual pair of the row solve's pre-split path (als_row_solve_params::R_scale): from the
        # largest |rating|, once per fit, here where the ratings are staged - they do not change between iterations,
        # so the replayed graph carries the same constant as the eager fit.  Both half steps pass it: the U-step takes
        # that path at k = 49 ... 64, the V-step whenever its gathered table (U) is small enough.
        self.rs_kw = {}
        if hasattr(self.be, "residual_scale"):
            vmax = cache.get(("max_abs_val", ku), lambda: float(torch.as_tensor(csr.vals).abs().max().item())
                             if csr.vals.shape[0] else 0.0)
            self.rs_kw = {"residual_scale": self.be.residual_scale(vmax)}
        uptr_h = cache.get(("indptr_h", ku), lambda: self.csr.indptr.cpu().numpy())
        iptr_h = cache.get(("indptr_h", ki), lambda: self.csc.indptr.cpu().numpy())
        # --- shards: contiguous row ranges balanced by predicted cost = ratings + c(k) * rows (about
        # half of a U-step row's time at cfg 4 is per row, not per rating, so rating-balanced shards of a skewed input
        # would be time-imbalanced); every rank derives the same tables from the row pointers.  The user shard is solved in u_chunks sub-ranges whose all-gathers overlap
        # the next sub-range's solve.  Factor storage is exactly [rows + 1, ld] (the extra row is the zero row).
        k, f32 = self.k, torch.float32
        self.u_chunks = max(1, int(os.environ.get("ALS_U_CHUNKS", self.U_CHUNKS))) if self.multi else 1
        self.row_cost = layout.row_cost_weight(k)
        self.ubounds, self.uchunks = layout.shard_bounds_nnz(uptr_h, self.world, self.u_chunks, self.row_cost)
        self.ibounds, _ = layout.shard_bounds_nnz(iptr_h, self.world, 1, self.row_cost)
        self.ub, self.ue = self.ubounds[self.rank]
        self.ib, self.ie = self.ibounds[self.rank]
        self.utasks = self._tasks_dev(cache, ku, uptr_h, self.ub, self.ue)
        self.itasks = self._tasks_dev(cache, ki, iptr_h, self.ib, self.ie)
        self.utasks_c = ([self._tasks_dev(cache, ku, uptr_h, b, e) for b, e in self.uchunks[self.rank]]
                         if self.u_chunks > 1 else None)
        nslots = max(self.utasks.nslots, self.itasks.nslots)
        slot_bytes = max(self.be.slot_bytes(k), self.be.slot_bytes(k, True) if self.v_f64 else 0)
        self.workspace = (torch.empty(nslots * slot_bytes // 4, dtype=f32, device=self.dev) if nslots else None)
        # Everything the host reads back per iteration lives in ONE 128-byte block: the history row (6 doubles at
        # byte 0) and the three status words (int32 at byte 64: row-solve status, sweep error, W-step status) - early
        # stopping then costs a single contiguous device-to-host copy per iteration instead of four small ones.
        self.ctrl = torch.zeros(128, dtype=torch.uint8, device=self.dev)
        self.hist_row = self.ctrl[0:48].view(torch.float64)
        words = self.ctrl[64:128].view(torch.int32)
        self.status, self.gs_err_word, self.w_bad = words[0:1], words[1:2], words[2:3]
        self.status_words = words[0:4]
        return np.diff(iptr_h).astype(np.float64)

    def _init_params(self, model, cache, ku, init_key, init_future):
        # --- parameters (scripts/als.py:329,360-376): numpy Generator on the host, same draw order
        f32, f64, device = torch.float32, torch.float64, self.dev
        mean0 = cache.get(("mean", ku), lambda: float(self.csr.vals.to(f64).mean().item()) if self.nnz
                          else float("nan"))                                                 # :360
        self.mu = torch.tensor([mean0], dtype=f64, device=device)

        def upload_init():
            U0, V0, W0 = init_future.result()
            return (torch.from_numpy(U0).to(device), torch.from_numpy(V0).to(device),
                    [torch.from_numpy(w).to(device) for w in W0])

        U0d, V0d, W0d = cache.get(init_key, upload_init)
        if model._fit_cache is not None:        # the cached initial state stays pristine
            U0d, V0d, W0d = U0d.clone(), V0d.clone(), [w.clone() for w in W0d]
        self.U, self.V = U0d[: self.m], V0d[: self.n]        # (without the zero row)
        self.b_u = torch.zeros(self.m, dtype=f32, device=device)
        self.b_i = torch.zeros(self.n, dtype=f32, device=device)
        self.b_i_prev = None            # b_i before the V-step of the running iteration, when a later step needs it
        self.W64 = dict(zip(self.feat_names, W0d))

    def _init_features(self, cache, features):
        if not self.feat_names:
            self.Xcat = self.X64 = self.Wcat = None
            self.Z = self.V                       # Z == V when there are no features
            return
        f32, device = torch.float32, self.dev

        def upload_features():
            return (torch.from_numpy(concat_features(features, self.feat_names)).to(device),
                    {f: torch.from_numpy(np.asarray(features[f], dtype=np.float64)).to(device)
                     for f in self.feat_names})
        fkey = ("features", tuple((f, cache.pin(features[f])) for f in self.feat_names), self.n)
        self.Xcat, self.X64 = cache.get(fkey, upload_features)
        self.Wcat = torch.zeros(self.Xcat.shape[1], self.ld, dtype=f32, device=device)
        self.Z = torch.zeros(self.n + 1, self.ld, dtype=f32, device=device)[: self.n]
        self._sync_wcat()

    def _init_item_reg(self, model, counts):
        # --- per-item regularisation (scripts/als.py:379-384, 243-259)
        if not model.pop_reg_mode:
            lam_v = np.full(self.n, float(model.lambda_v))
        else:
            lam_v = model.lambda_v / np.sqrt(counts + 1.0)
        self.lam_v_row = torch.from_numpy(lam_v.astype(np.float32)).to(self.dev)

    def _upload_graph(self, model, S_csr):
        device, f64 = self.dev, torch.float64
        S_ptr = _to_dev(S_csr[0], device, torch.int64)
        S_idx = _to_dev(S_csr[1], device, torch.int32)
        S_val = _to_dev(S_csr[2], device, torch.float32)
        if model._validate_S:                 # caller-supplied graph: checked once, on the device
            if S_ptr.numel() != self.n + 1:
                raise ValueError(f"similarity graph S has {S_ptr.numel() - 1} rows; expected {self.n}")
            _validate_graph(S_ptr, S_idx, S_val, self.n)
        if len(S_csr) > 3:
            D = _to_dev(S_csr[3], device, torch.float32)
        else:                       # D = S.sum(axis=1) (scripts/als.py:357); segment sums from an fp64
            # prefix sum: deterministic (index_add_ would use float atomics)
            csum = torch.zeros(S_val.numel() + 1, dtype=f64, device=device)
            csum[1:] = torch.cumsum(S_val.to(f64), 0)
            D = (csum[S_ptr[1:]] - csum[S_ptr[:-1]]).to(torch.float32)
        return S_ptr, S_idx, S_val, D, S_ptr.cpu().numpy(), S_idx.cpu().numpy()

    def _level_schedule(self, ptr, idx, active, lo, hi):
        if self.native:
            sched, wait = layout.build_level_schedule_native(self.be.lib, ptr, idx, active, lo, hi,
                                                             want_wait=self.gs_dataflow)
        else:
            sched = layout.build_level_schedule(ptr, idx, active, lo, hi)
            wait = layout.wait_edges(ptr, idx, sched.level) if self.gs_dataflow else None
        return (sched, torch.from_numpy(sched.items).to(self.dev),
                torch.from_numpy(wait).to(self.dev) if wait is not None else None)

    def _init_graph(self, model, cache, S_csr, ki, active):
        # --- graph: the similarity CSR, the Laplacian's diagonal, the level schedule and the dataflow sweep's buffers
        self.S_ptr = self.S_idx = self.S_val = self.diag_extra = self.sched = self.sched_items = None
        self.S_idx_wait = self.gs_publish = self.gs_err = self.gs_nondep = None
        if not self.use_graph:
            return
        kg = cache.pin(S_csr)
        self.S_ptr, self.S_idx, self.S_val, D, ptr, idx = cache.get(("graph", kg, bool(model._validate_S)),
                                                                    lambda: self._upload_graph(model, S_csr))
        self.diag_extra = np.float32(model.alpha) * D
        lo, hi = (0, self.n) if (self.multi and self.gs_mode == "levels") else (self.ib, self.ie)
        self.sched, self.sched_items, wait_dev = cache.get(("sched", kg, ki, lo, hi, bool(self.gs_dataflow)),
                                                           lambda: self._level_schedule(ptr, idx, active, lo, hi))
        if self.gs_dataflow:
            f32 = torch.float32
            self.S_idx_wait = wait_dev
            self.gs_publish = torch.empty(self.n, self.ld, dtype=f32, device=self.dev)       # same shape as V
            self.gs_err = self.gs_err_word
            # Neighbour sums that do not depend on the sweep can be formed for all items by a parallel launch
            # before it (same sums, same order).  On graphs without hubs the in-sweep gather hides behind the
            # dependency waits and the extra launch only costs (cfg 4, sampled graph: 1.79 vs 1.46 ms); with hub
            # rows it pays (exact top-50 graph, rows of up to 3700 neighbours: 2.43 vs 2.75 ms).  Default: on
            # when the longest row of S has 1024 neighbours or more; ALS_GS_NONDEP=0 / 1 forces it.
            nd_env = os.environ.get("ALS_GS_NONDEP")
            hubs = bool(ptr.size > 1 and int(np.diff(ptr).max()) >= 1024)
            if nd_env == "1" or (nd_env is None and hubs):
                self.gs_nondep = torch.empty(self.n, self.ld, dtype=f32, device=self.dev)

    def _local(self, *row_shape, dtype=None):
        """A zero-filled by-product array over this rank's items (see `_init_byproducts`)."""
        r0, nloc = self.local_rows
        t = torch.zeros((nloc,) + row_shape, dtype=dtype or (torch.float64 if self.v_f64 else torch.float32),
                        device=self.dev)
        return _RowShift(t, r0, int(np.prod(row_shape)) if row_shape else 1) if self.native else t

    def _init_byproducts(self):
        # By-products of the V-step exist for this rank's items only ([ib, ie): n / world rows instead of n - the
        # item Grams and Cholesky factors are n * ld^2 floats each, 65 GB at BASELINE configs[4]); the kernels index
        # them with absolute item ids through a shifted base pointer (_RowShift).  The numpy stand-in of the CPU
        # tests indexes tensors directly, so it keeps full-size arrays.
        self.local_rows = (self.ib, self.ie - self.ib) if self.native else (0, self.n)
        nloc = self.local_rows[1]
        self.factor = self._local(self.ld * self.ld) if self.use_graph else None
        self.sumr = self._local() if self.use_graph else None
        need_byproducts = self.use_graph or bool(self.feat_names)
        self.rhs_out = self._local(self.ld) if need_byproducts else None
        self.colsum_out = self._local(self.ld) if need_byproducts else None
        self.gram = self._local(self.ld, self.ld) if self.feat_names else None
        # Rank-local by-products scale with the rank's ITEM COUNT (factor / gram: ld^2 per item), the shards are cut by
        # cost (ratings + c rows): when item ids correlate with popularity the tail shard holds more than n / world
        # items.  Say so instead of letting the "n / world rows" memory statement fail silently.
        elt = 8 if self.v_f64 else 4
        self.byproduct_bytes = nloc * elt * ((self.ld * self.ld if self.use_graph else 0)
                                             + (self.ld * self.ld if self.feat_names else 0)
                                             + (2 * self.ld if need_byproducts else 0))
        if self.multi and self.native:
            even = -(-self.n // self.world)
            logger.info("rank %d: %d of %d items, %.2f GB of V-step by-products", self.rank, nloc, self.n,
                        self.byproduct_bytes / 1e9)
            if nloc > 1.5 * even + 64:
                logger.warning("rank %d holds %d items (even share %d): its V-step by-products take %.2f GB, %.1fx the "
                               "even share - item ids correlate with popularity; shards are balanced by cost, not by "
                               "item count", self.rank, nloc, even, self.byproduct_bytes / 1e9, nloc / max(even, 1))
        # what the chosen statistics path (`_decide_paths`) reads besides these
        fused = self.fused_stats or self.fused_feat_stats
        self.stat_rows = self._local(2, dtype=torch.float32) if fused else None
        self.sumr2 = self._local() if fused and (self.use_graph or self.fused_feat_stats) else None
        self.lam_eff = ((self.lam_v_row + np.float32(EPS) + self.diag_extra).contiguous()
                        if fused and self.use_graph else None)
        if self.fused_feat_stats and not self.use_graph:
            self.sumr = self._local()

    def _init_wstep(self):
        # the W-step's persistent buffers: with features only (iteration 0 then always runs the W-step)
        self.H = self.feat_off = self.feat_off_host = self.w_status = None
        if not self.feat_names:
            return
        r0, nloc = self.local_rows
        H = torch.zeros(len(self.feat_names), nloc, self.ld, dtype=torch.float64 if self.v_f64 else torch.float32,
                        device=self.dev)
        self.H = _RowShift(H, r0, self.ld) if r0 or nloc != self.n else H
        self.feat_off_host = np.concatenate([[0], np.cumsum(self.feat_dims)]).astype(np.int32)
        self.feat_off = torch.from_numpy(self.feat_off_host).to(self.dev)
        self.w_status = torch.zeros(1, dtype=torch.int32, device=self.dev)    # (w_bad: sticky, in self.ctrl)

    def _init_scratch(self, model):
        # --- stats scratch
        f64 = torch.float64
        self.stats = torch.zeros(2, dtype=f64, device=self.dev)
        self.ss = torch.zeros(4, dtype=f64, device=self.dev)
        self.hist = torch.zeros(max(model.n_iters, 1), 6, dtype=f64, device=self.dev)
        self._graphs = {}
        self._stage = {}                # receive buffers of _allgather_rows, one per (tensor, rows per rank)
        self.graphs_captured = 0
        self.replay_ok = True           # (diagnostics: set False to force eager iterations)
        self.iters_run = 0

    # ------------------------------------------------------------- helpers
    def _padded_host(self, A64: np.ndarray) -> np.ndarray:
        """[rows + 1, ld] fp32 array whose first rows are the factor matrix: the extra last row stays zero for
        ever - als_row_solve points ratings past the end of a row at it (F_zero_row)."""
        out = np.zeros((A64.shape[0] + 1, self.ld), dtype=np.float32)
        out[: A64.shape[0], : self.k] = A64
        return out

    def _sync_wcat(self):
        self._concat_w(self.feat_names, self.feat_dims, out=self.Wcat)

    def _allgather_rows(self, t: torch.Tensor, bounds, async_op: bool = False, tag=None):
        """All-gather of the contiguous, unevenly sized row shards `bounds[r] = (begin, end)` of `t`: every rank
        contributes `per` rows (the longest shard) in one all_gather_into_tensor - RCCL and gloo both need equal
        sizes -, `finish()` copies the other ranks' rows into place (`tag` keeps exchanges that are in flight
        together - the sub-ranges of the U-step - on separate receive buffers).  No staging copy of the own rows: rank r sends
        the window t[s_r : s_r + per] with s_r = min(begin_r, rows - per), which contains its shard (what else is
        in the window is ignored by the receivers).  The receive buffer is allocated once per (tensor, per).
        Returns finish (called at once unless async_op)."""
        if not self.multi:
            return None
        rows = t.shape[0]
        per = min(max(max(hi - lo for lo, hi in bounds), 1), rows)
        starts = [min(lo, rows - per) for lo, _ in bounds]
        tail = tuple(t.shape[1:])
        key = (tag, t.data_ptr(), per, tail, t.dtype)
        stage = self._stage.get(key)
        if stage is None:
            stage = self._stage[key] = torch.empty((self.world, per) + tail, dtype=t.dtype, device=t.device)
        s0 = starts[self.rank]
        work = dist.all_gather_into_tensor(stage.view(-1), t[s0:s0 + per].reshape(-1), group=self.pg,
                                           async_op=async_op)

        def finish():
            if work is not None:
                work.wait()
            for r, (lo, hi) in enumerate(bounds):
                if r != self.rank and hi > lo:
                    t[lo:hi] = stage[r, lo - starts[r]: hi - starts[r]]
        if async_op:
            return finish
        finish()
        return None

    def _global_rank(self, r: int) -> int:
        return r if self.pg is None else dist.get_global_rank(self.pg, r)

    def _allreduce(self, t: torch.Tensor):
        if self.multi:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg)

    def _read_ctrl(self):
        """(history row, status words) of the last iteration: one contiguous 128-byte device-to-host copy.
        With several ranks the status words are first reduced (MAX) over the group, so that every rank takes the
        same decision - all raise LinAlgError / SweepNotResident (and refit) together, or none does; a rank that
        left the iteration loop alone would leave the others waiting in their next collective."""
        if self.multi:
            dist.all_reduce(self.status_words, op=dist.ReduceOp.MAX, group=self.pg)
        c = self.ctrl.cpu()
        return c[0:48].view(torch.float64).numpy(), c[64:76].view(torch.int32).numpy()

    def _check_status(self, words=None):
        if words is None:
            words = self._read_ctrl()[1]
        # the sweep's error word first: it is sticky, every later sweep bails out at its first wait, and whatever
        # else went wrong afterwards (NaN factors -> "not positive definite") is a consequence
        if self.gs_dataflow and int(words[1]):
            raise SweepNotResident("Gauss-Seidel dataflow sweep: a dependency wait exceeded its bound (the persistent "
                                   "launch was not resident as a whole)")
        if int(words[2]):
            raise np.linalg.LinAlgError("W-step normal equations of a feature are not positive definite")
        bad = int(words[0])
        if bad:
            self.status.zero_()
            raise np.linalg.LinAlgError(
                f"normal equations of row {bad - 1} are not positive definite")   # scripts/helpers.py:19

    @contextlib.contextmanager
    def _tick(self, name):
        """Context manager recording a (name, start, end) event pair on the current stream."""
        if self.timers is None:
            yield
            return
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        try:
            yield
        finally:
            b.record()
            self.timers.append((name, a, b))

    # ---------------------------------------------------------- half steps
    def user_step(self):
        """scripts/als.py:414-433 on this rank's user shard, then all-gather.

        With several ranks the shard is solved in U_CHUNKS contiguous sub-ranges; the all-gather of a
        finished sub-range (async, on the collective stream) overlaps the solve of the next one.
        """
        md = self.model
        kw = dict(k=self.k, ld=self.ld, side=self.csr, F=self.Z, zero_row=self.n, bias_self=self.b_u,
                  bias_other=self.b_i, mu=self.mu, lam=md.lambda_u, lam_row=None, lam_b=md.lambda_bu,
                  lam_b_row=None, rhs_extra=None, diag_extra=None, X_out=self.U, bias_out=self.b_u,
                  gram_out=None, factor_out=None, rhs_out=None, colsum_out=None, sumr_out=None,
                  status=self.status, workspace=self.workspace, **self.rs_kw)
        if self.u_chunks == 1:
            with self._tick("row_solve_user"):
                self.be.row_solve(tasks=self.utasks, **kw)
            self._allgather_rows(self.U, self.ubounds)
            self._allgather_rows(self.b_u, self.ubounds)
            return
        pending = []
        with self._tick("row_solve_user"):
            for c in range(self.u_chunks):
                if self.utasks_c[c].ntasks or self.utasks_c[c].nlong:
                    self.be.row_solve(tasks=self.utasks_c[c], **kw)
                cb = [self.uchunks[r][c] for r in range(self.world)]        # sub-range c of every rank's shard
                pending.append(self._allgather_rows(self.U, cb, async_op=True, tag=c))
                pending.append(self._allgather_rows(self.b_u, cb, async_op=True, tag=c))
        with self._tick("allgather_user_wait"):
            for finish in pending:
                finish()

    def item_step(self, want_gram: bool):
        """scripts/als.py:436-466 on this rank's item shard, then all-gather.

        The feature part of Z is deliberately not used here (reference quirk,
        :447,:465): F = U, and the bias update uses V, not Z.
        """
        md = self.model
        common = dict(k=self.k, ld=self.ld, side=self.csc, F=self.U, zero_row=self.m, bias_self=self.b_i,
                      bias_other=self.b_u, mu=self.mu, lam=0.0, lam_row=self.lam_v_row,
                      lam_b=md.lambda_bi, lam_b_row=None, rhs_extra=None,
                      gram_out=self.gram if want_gram else None, status=self.status,
                      tasks=self.itasks, workspace=self.workspace, **self.f64kw, **self.rs_kw)
        if not self.use_graph:
            with self._tick("row_solve_item"):
                self.be.row_solve(diag_extra=None, X_out=self.V, bias_out=self.b_i, factor_out=None,
                                  rhs_out=self.rhs_out if want_gram else None,
                                  colsum_out=self.colsum_out if want_gram else None,
                                  sumr_out=self.sumr if self.fused_feat_stats else None,
                                  sumr2_out=self.sumr2 if self.fused_feat_stats else None,
                                  stat_out=self.stat_rows if self.fused_stats else None, **common)
        else:
            # phase A (parallel): Gram, rhs, Cholesky factor of every item of the shard
            with self._tick("row_solve_item"):
                self.be.row_solve(diag_extra=self.diag_extra, X_out=None, bias_out=None,
                                  factor_out=self.factor, rhs_out=self.rhs_out, colsum_out=self.colsum_out,
                                  sumr_out=self.sumr,
                                  sumr2_out=self.sumr2 if (self.fused_stats or self.fused_feat_stats) else None,
                                  **common)
            # phase B (sequential in levels): Gauss-Seidel sweep with live V (:458)
            if self.multi and self.gs_mode == "exact":
                # shards in rank order; the broadcast hands shard r's new rows to everybody before shard
                # r + 1 starts (stream-ordered on every rank)
                with self._tick("gs_sweep"):
                    for r in range(self.world):
                        if r == self.rank:
                            self._gs_sweep()
                        lo, hi = self.ibounds[r]
                        if hi > lo:
                            dist.broadcast(self.V[lo:hi], src=self._global_rank(r), group=self.pg)
                self._allgather_rows(self.b_i, self.ibounds)
                return
            with self._tick("gs_sweep"):
                self._gs_sweep()
        self._allgather_rows(self.V, self.ibounds)
        self._allgather_rows(self.b_i, self.ibounds)

    def _gs_sweep(self):
        md = self.model
        off = self.sched.offsets
        exact_multi = self.multi and self.gs_mode == "levels"
        kw = dict(k=self.k, ld=self.ld, S_ptr=self.S_ptr, S_idx=self.S_idx, S_val=self.S_val,
                  alpha=md.alpha, factor=self.factor, rhs=self.rhs_out, colsum=self.colsum_out,
                  sumr=self.sumr, indptr=self.csc.indptr, lam_b=md.lambda_bi, lam_b_row=None,
                  V=self.V, bias=self.b_i, **self.f64kw)
        if self.fused_stats:
            kw.update(sumr2=self.sumr2, lambda_eff=self.lam_eff, stat_out=self.stat_rows)
        if self.gs_dataflow:
            self.be.gs_dataflow(items=self.sched_items, S_idx_wait=self.S_idx_wait, publish=self.gs_publish,
                                err=self.gs_err, nondep=self.gs_nondep, **kw)
            return
        if not exact_multi and self.has_gs_levels:
            # no collective between levels: the whole sweep is one C call (one launch per level)
            self.be.gs_levels(offsets=np.ascontiguousarray(off, dtype=np.int64), items=self.sched_items, **kw)
            return
        for lv in range(len(off) - 1):
            items = self.sched_items[off[lv]:off[lv + 1]]
            if exact_multi:
                it_np = self.sched.items[off[lv]:off[lv + 1]]
                lo = int(np.searchsorted(it_np, self.ib))
                hi = int(np.searchsorted(it_np, self.ie))
                mine = items[lo:hi]
            else:
                mine = items
            if mine.numel():
                self.be.gs_level(items=mine, **kw)
            if exact_multi:
                self._exchange_level(items, it_np)

    def _exchange_level(self, items: torch.Tensor, it_np: np.ndarray):
        """Exact multi-GPU sweep: publish this level's freshly solved V rows."""
        ends = np.array([hi for _, hi in self.ibounds], dtype=np.int64)
        owner = np.searchsorted(ends, it_np, side="right")          # rank whose [begin, end) holds the item
        cnt = np.bincount(owner, minlength=self.world)
        cmax = int(cnt.max())
        if cmax == 0:
            return
        lo = int(np.searchsorted(it_np, self.ib))
        buf = torch.zeros(cmax, self.ld, dtype=torch.float32, device=self.dev)
        n_mine = int(cnt[self.rank])
        if n_mine:
            buf[:n_mine] = self.V[items[lo:lo + n_mine].long()]
        allb = torch.empty(self.world * cmax, self.ld, dtype=torch.float32, device=self.dev)
        dist.all_gather_into_tensor(allb.view(-1), buf.view(-1), group=self.pg)
        start = 0
        for r in range(self.world):
            c = int(cnt[r])
            if c and r != self.rank:
                self.V[items[start:start + c].long()] = allb[r * cmax:r * cmax + c]
            start += c

    # --------------------------------------------------------------- W step
    def w_step(self, b_i_old: torch.Tensor):
        """scripts/als.py:468-501 without the N_obs x (d k) design matrix.

        With G_i = U_i^T U_i (the item Gram of this iteration's V-step) the
        reference's normal equations are
            A_f = sum_i (x_i x_i^T) (x) G_i + (lambda_f + 1e-10) I
            b_f = sum_i x_i (x) (g_i + G_i xw_{f,i}),   g_i = U_i^T residual_i
        and g_i = U_i^T rho_i - G_i z_i follows from the V-step by-products
        (rhs, column sums), so no extra pass over the ratings is needed.  The
        Jacobi-across-features quirk (:474-489) and the lambda=0-for-missing
        quirk (:497) are kept.  A_f / b_f come from the HIP kernels of
        w_step.hip (als_w_normal_equations) in fp64 and are solved by the blocked
        fp64 Cholesky of spd_solve.hip (als_spd_solve_f64).
        """
        md = self.model
        k, ld = self.k, self.ld
        Wold = torch.cat([self.W64[f] for f in self.feat_names], dim=0).contiguous() if self.v_f64 else self.Wcat
        self.be.w_item_vectors(k=k, ld=ld, item_begin=self.ib, item_end=self.ie, gram=self.gram,
                               rhs=self.rhs_out, colsum=self.colsum_out, V=self.V, b_new=self.b_i,
                               b_old=b_i_old, X=self.Xcat, feat_off=self.feat_off, W=Wold, H=self.H, **self.f64kw)
        newW = {}
        for fi, (f, d) in enumerate(zip(self.feat_names, self.feat_dims)):
            A_full, B_full = self.be.w_accumulate(k=k, ld=ld, item_begin=self.ib, item_end=self.ie,
                                                  gram=self.gram, X=self.Xcat, H=self.H, feat_index=fi,
                                                  feat_col0=int(self.feat_off_host[fi]), feat_d=d, **self.f64kw)
            if self.multi:
                self._allreduce(A_full)
                self._allreduce(B_full)
            x = self.be.spd_solve(A_full, B_full, float(md.lambda_w.get(f, 0.0)) + EPS, self.w_status)
            torch.maximum(self.w_bad, self.w_status, out=self.w_bad)     # no host round trip inside an iteration
            newW[f] = x.reshape(d, k)
        for f in self.feat_names:           # into the persistent buffers (Jacobi across features: all solves first);
            self.W64[f].copy_(newW[f])      # a tensor born inside a captured iteration lives in the graph's pool
        self._sync_wcat()

    # ---------------------------------------------------------------- stats
    def stats_step(self, it: int):
        """scripts/als.py:503-517: mu update and the five history series."""
        if self.feat_names:
            self.be.compose_z(self.V, self.Xcat, self.Wcat, self.Z)              # :504
        with self._tick("residual_stats"):
            if self.fused_stats:        # per-item (sum d, sum d^2) written by the V-step / the sweep
                self.be.sum_pairs(self.stat_rows, self.stats)
            elif self.fused_feat_stats:  # per-item closed form with the final Z (features present)
                self.be.item_stats(k=self.k, ld=self.ld, item_begin=self.ib, item_end=self.ie, gram=self.gram,
                                   rhs=self.rhs_out, colsum=self.colsum_out, sumr=self.sumr, sumr2=self.sumr2,
                                   indptr=self.csc.indptr, Z=self.Z, b_new=self.b_i, b_old=self.b_i_prev,
                                   stat_out=self.stat_rows, **self.f64kw)
                self.be.sum_pairs(self.stat_rows, self.stats)
            else:
                self.be.residual_stats(k=self.k, ld=self.ld, side=self.csr, U=self.U, Z=self.Z, b_u=self.b_u,
                                       b_i=self.b_i, mu=self.mu, tasks=self.utasks, out=self.stats)
        self._allreduce(self.stats)
        h = self.hist_row                 # fixed address: the iteration can be replayed as a captured graph
        if self.has_history_row:
            self.be.history_row(U=self.U, V=self.V, b_u=self.b_u, b_i=self.b_i, stats=self.stats, nnz=self.nnz,
                                mu=self.mu, row=h)
        else:
            for j, t in enumerate((self.U, self.V, self.b_u, self.b_i)):
                self.be.sumsq(t, self.ss[j:j + 1])
            mean_d = self.stats[0] / self.nnz
            self.mu += mean_d
            h[0] = torch.sqrt(torch.clamp(self.stats[1] / self.nnz - mean_d * mean_d, min=0.0))
            h[1:5] = torch.sqrt(self.ss)
            h[5] = self.mu[0]
        if it is not None:
            self.hist[it].copy_(h)

    # ------------------------------------------------------------------ run
    def iteration(self, it: int, n_iters: int):
        """One full ALS iteration (scripts/als.py:408-517), asynchronous on the stream."""
        md = self.model
        if self.dev.type == "cuda" and torch.cuda.current_device() != self.dev.index and self.dev.index is not None:
            with torch.cuda.device(self.dev):          # callers that drive iterations themselves (bench.py)
                return self.iteration(it, n_iters)
        do_w = bool(self.feat_names) and ((it % md.update_w_every == 0) or (it == n_iters - 1))   # :468
        if self.model._hip_graph and self.replay_ok and not self.multi and self.timers is None and it > 0:
            self._replay(do_w)
            self.hist[it].copy_(self.hist_row)
        else:
            self._iteration_body(do_w, it)
        self.iters_run = it + 1

    def _iteration_body(self, do_w: bool, it):
        # Z is current here: stats_step recomposes it after every V / W update
        self.user_step()
        b_i_old = self.b_i.clone() if (do_w or self.fused_feat_stats) else None
        self.b_i_prev = b_i_old
        self.item_step(want_gram=do_w or self.fused_feat_stats)
        if do_w:
            with self._tick("w_step"):
                self.w_step(b_i_old)
        self.stats_step(it)

    def _replay(self, do_w: bool):
        """The iteration as a captured HIP graph (one per W-step / no-W-step variant): every launch of the
        body - kernels of libals_hip.so on the capture stream, memsets, the few torch tensor ops - becomes a
        graph node; later iterations replay it with one submission.  The first iteration always runs eagerly
        (allocations, lazy initialisation, occupancy queries)."""
        g = self._graphs.get(do_w)
        if g is None:
            torch.cuda.synchronize(self.dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._iteration_body(do_w, None)
            self._graphs[do_w] = g
            self.graphs_captured += 1
        g.replay()

    def run(self, tol, min_iters, verbose):
        md = self.model
        n_iters = int(md.n_iters)
        rm = md.history["train_rmse"]
        base_len = len(rm)
        # Captured-graph replay (hip_graph=True) also serves fits with early stopping: the host reads ONE contiguous
        # 128-byte block per iteration between the replays.  (Round 1 / early round 2 had replay limited to tol=None
        # because "host read-backs corrupt later replays"; the real cause was the sweep's hipMemsetD32Async: with the
        # two iteration graphs alive - W-step / no-W-step variant - each holding a memset node, replays went wrong
        # from the first switch back, reads or no reads.  The reset is a kernel now (gs_sweep.hip) and replay is
        # bitwise the eager fit over 120 iterations with per-iteration reads: profiles/graph_early_stop_stress.py,
        # tests/test_gpu_parity.py::test_hip_graph_replay_with_early_stopping_reads.)
        self.replay_ok = True
        if self.feat_names:
            self.be.compose_z(self.V, self.Xcat, self.Wcat, self.Z)              # :411
        seen = list(rm)                 # train RMSE so far (earlier fits of the same model + this one)
        for it in range(n_iters):
            self.iteration(it, n_iters)
            if tol is not None:
                # one read-back per iteration: the history row (-> the stopping rule) and the status words
                row, words = self._read_ctrl()
                seen.append(float(row[0]))
                if it + 1 >= min_iters:                                           # :520-523
                    self._check_status(words)
                    if len(seen) >= 3 and seen[-3] - seen[-1] <= tol:
                        if verbose > 0:
                            logger.info("Early stopping at iter %d; dRMSE <= %.3g", it + 1, tol)
                        break
        self._check_status()
        self._graphs.clear()            # captured iteration graphs are not needed past the fit

    # --------------------------------------------------------------- export
    def export(self, model):
        k = self.k
        model.U = self.U[:, :k].to(torch.float64).cpu().numpy()
        model.V = self.V[:, :k].to(torch.float64).cpu().numpy()
        model.b_u = self.b_u.to(torch.float64).cpu().numpy()
        model.b_i = self.b_i.to(torch.float64).cpu().numpy()
        model.mu = float(self.mu.item())
        for f in self.feat_names:
            model.W[f] = self.W64[f].cpu().numpy()
        h = self.hist[: self.iters_run].cpu().numpy()
        for j, key in enumerate(("train_rmse", "U_norm", "V_norm", "bu_norm", "bi_norm")):
            model.history[key].extend(float(x) for x in h[:, j])
