"""HIP backend: torch tensors in, C-ABI calls out (include/als_hip.h).

torch is used for what it is good at here - device memory, streams, and the
process group.  All arithmetic of the per-rating / per-row hot path happens in
the hand-written kernels behind the C ABI.  The engine (engine.py) talks to this
object only through the methods below, so that the sharding / collective logic
can be exercised on CPU under gloo with a stand-in solver living in tests/.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import torch

from . import _hip


def _p(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class HipBackend:
    name = "hip"

    GRAM_MODES = {"f32": 0, "f16x2": 1, "f64": 2}
    COND_LIMIT = 300.0
    SOLVE_DTYPES = ("auto", "refine", "float32", "float64")
    REFINE_MAX_STEPS = 5
    PLANES_MAX_FLOATS = 16 << 20       # 64 MiB table: V / Z of every BASELINE shape, never U
    PLANES_MAX_FLOATS_K128 = (1 << 31) - 1     # k = 128: any table als_row_solve accepts (element offsets < 2^31)

    def __init__(self, device: torch.device, gram: str = "f16x2", solve_dtype: str = "auto"):
        if gram not in ("f32", "f16x2"):
            raise ValueError("gram must be 'f16x2' or 'f32'")
        if solve_dtype not in self.SOLVE_DTYPES:
            raise ValueError("solve_dtype must be 'auto', 'refine', 'float32' or 'float64'")
        # solve_dtype="float64": Gram, Cholesky and substitutions of every row in fp64 (ALS_GRAM_F64); `gram` then
        # has no effect
        self.solve_dtype = solve_dtype
        self.gram_mode = self.GRAM_MODES["f64" if solve_dtype == "float64" else gram]
        if device.type != "cuda":
            raise RuntimeError("HipBackend needs a ROCm device (torch device type 'cuda'); "
                               "there is no CPU path in the product")
        self.lib = _hip.load()
        self.device = device
        self._sumsq_partials = torch.empty(self.lib.als_sumsq_partials(), dtype=torch.float64,
                                           device=device)
        self._stats_partials: Optional[torch.Tensor] = None
        self._ws: dict = {}                # workspaces of the library calls by name (`_workspace`): uint8, grow-only
        self._rec_ws: Optional[torch.Tensor] = None        # item-slice lists of als_recommend_topk* (`_recommend`)
        self._rank_ws: Optional[torch.Tensor] = None       # item-slice counts of als_rank_count* (`_rank`)
        # operand scale of the f16x2 Gram ({S, 1 / S^2} of the gathered factor matrix + two working words that stay
        # zero between calls: als_factor_scale); one per backend - calls on one stream run in order
        self._fscale = torch.zeros(4, dtype=torch.float32, device=device)
        self.ablate = int(os.environ.get("ALS_ABLATE", "0"))   # phase ablation of als_row_solve (profiles/ablate.sh)
        # scratch for the pre-split operands of the Gram (row_solve; keyed by table size) and the largest gathered table
        # (floats) it is used for; ALS_PLANES=0 switches the path off
        self._planes: dict = {}
        self.planes_max_floats = 0 if os.environ.get("ALS_PLANES", "1") == "0" else self.PLANES_MAX_FLOATS
        self.planes_max_floats_k128 = self.PLANES_MAX_FLOATS_K128 if os.environ.get("ALS_PLANES_K128") == "1" else 0
        # solve_dtype="auto": rows whose condition estimate (two lower bounds of cond_2 from their own fp32
        # factorisation: the pivot ratio (max L_ii / min L_ii)^2 and (trace(G) / rank + lambda) / min L_ii^2, both over
        # the pivots of the real system - the padding of k to a multiple of 16 has no say) exceeds
        # COND_LIMIT are redone in fp64 by the same call, as are rows whose closed-form residual statistics cancel to
        # fewer than three digits.  Calibration (profiles/r03_cond_estimates.txt): rows of cfg 4 / cfg 3 stay below
        # 5, of cfg 5 (k = 128, |z| up to 3) below 170 - no row of the BASELINE workloads is redone -, the
        # lambda = 1e-2 fixture 14 ... 1300, lambda = 1e-4 10^3 ... 3 10^5.  A row that stays fp32 has a relative
        # error (max norm) of up to about 55 * estimate * 2^-24 - measured: 3.3e-4 at an estimate of 100, a low-rank
        # row of 4100 ratings, so about 1e-3 at COND_LIMIT; 1e-5 on well-conditioned rows
        # (tests/test_gpu_row_auto.py, profiles/row_auto_kernel_test_margins.json).
        # ALS_COND_LIMIT overrides.
        # solve_dtype="refine": "auto" in everything above - same estimate, same limit, same flagged rows - but a plain
        # solve call (the U-step) hands the flagged rows to als_row_solve_refine: a few steps of iterative refinement
        # on the row's own fp32 factor, the residual in fp64 from the ratings.  Rows that do
        # not contract within refine_max_steps, whose fp32 factorisation breaks down or that are longer than
        # SPLIT_CHUNK fall back to the fp64 kernel: _fallback_count of the _redo_count flagged rows; _refine_steps[s]
        # counts the rows accepted after s steps.  All three describe the last row_solve call.
        self.cond_limit = (float(os.environ.get("ALS_COND_LIMIT", self.COND_LIMIT))
                           if solve_dtype in ("auto", "refine") else 0.0)
        self._redo_count = torch.zeros(1, dtype=torch.int32, device=device)
        self._redo_rows: dict = {}         # rows of the orientation -> int32 list buffer
        self.refine_max_steps = self.REFINE_MAX_STEPS
        self._fallback_count = torch.zeros(1, dtype=torch.int32, device=device)
        self._fallback_rows: dict = {}
        self._refine_steps = torch.zeros(9, dtype=torch.int32, device=device)
        self.cond_probe: Optional[torch.Tensor] = None     # diagnostics: float32 [nrows], receives every row's estimate

    # -- helpers -------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _check(rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{what} failed with status {rc} (see ALS_E_* in include/als_hip.h)")

    def _workspace(self, name: str, need: int):
        """Pointer to the workspace `name` of at least `need` bytes - owned here, grown when a call needs more, never
        shrunk; None for need == 0 (the library then takes NULL)."""
        if need <= 0:
            return None
        buf = self._ws.get(name)
        if buf is None or buf.numel() < need:
            buf = self._ws[name] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return _p(buf)

    @staticmethod
    def _seen(seen_ptr, seen_idx):
        """The seen CSR as the library takes it: (None, None) when no row has an entry (and there is no storage to
        point at)."""
        if seen_idx is not None and seen_idx.numel() == 0:
            return None, None
        return _p(seen_ptr), _p(seen_idx)

    def _bitmap(self, allow: Optional[torch.Tensor], n: int):
        """Pointer to the allow bitmap of a call over n rows, checked; None allows every row (NULL).  The kernels
        index the words by row: a short bitmap would be an out-of-bounds read."""
        if allow is not None and (allow.dtype != torch.int32 or not allow.is_cuda or not allow.is_contiguous()
                                  or allow.numel() < (n + 31) // 32):
            raise ValueError(f"allow bitmap must be a contiguous int32 device tensor of {(n + 31) // 32} words")
        return _p(allow)

    def slot_bytes(self, k: int, f64: bool = False) -> int:
        """Bytes of one partial slot of a split row (fp64 calls keep an fp64 image per segment)."""
        if f64 or self.gram_mode == self.GRAM_MODES["f64"]:
            return int(self.lib.als_partial_slot_bytes_f64(k))
        return int(self.lib.als_partial_slot_bytes(k))

    # -- K1 ------------------------------------------------------------------
    @staticmethod
    def residual_scale(max_abs_val: float) -> float:
        """als_row_solve_params::R_scale for ratings of magnitude up to `max_abs_val`: the power of two that puts
        max_abs_val in [2^9, 2^10), clamped to 2^-126 ... 2^126 so that the scale and its inverse are normal fp32
        numbers; 1.0 for a side without ratings (0, or not finite).  The pre-split path of the row solve rounds
        (residual * scale) to two fp16 terms: 2^6 of headroom for mu and the biases below the fp16 overflow, a normal
        low term down to 2^-13 of the largest rating.  A per-fit constant: the ratings do not change between
        iterations, so it needs no device read and is the same under graph replay as in the eager fit."""
        v = float(max_abs_val)
        if not (0.0 < v < float("inf")):
            return 1.0
        e = math.frexp(v)[1] - 1                     # v in [2^e, 2^(e+1))
        return math.ldexp(1.0, max(-126, min(126, 9 - e)))

    def row_solve(self, *, k, ld, side, F, zero_row, bias_self, bias_other, mu, lam, lam_row, lam_b,
                  lam_b_row, rhs_extra, diag_extra, X_out, bias_out, gram_out, factor_out,
                  rhs_out, colsum_out, sumr_out, status, tasks, workspace, sumr2_out=None, stat_out=None,
                  f64=False, residual_scale=0.0):
        """`f64`: this call in fp64 whatever the backend's mode, by-product arrays (gram_out, factor_out, rhs_out,
        colsum_out, sumr_out, sumr2_out) being DOUBLE tensors (the engine's fp64 V-step).
        `residual_scale`: als_row_solve_params::R_scale, `residual_scale(max |side.vals|)` - read by the pre-split
        path alone; 0 leaves its residual pair unscaled (ratings of order 1 ... 10^3)."""
        p = _hip.RowSolveParams()
        p.k, p.ld, p.nrows, p.F_zero_row = k, ld, side.nrows, int(zero_row)
        p.reserved0 = self.ablate          # 0 in production; profiling builds of bench.py set it
        p.gram_mode = self.GRAM_MODES["f64"] if f64 else self.gram_mode
        p.byproducts_f64 = int(bool(f64))
        p.indptr, p.indices, p.vals = _p(side.indptr), _p(side.indices), _p(side.vals)
        p.F, p.bias_self, p.bias_other, p.mu = _p(F), _p(bias_self), _p(bias_other), _p(mu)
        p.lambda_scalar, p.lambda_row = float(lam), _p(lam_row)
        p.lambda_bias_scalar, p.lambda_bias_row = float(lam_b), _p(lam_b_row)
        p.rhs_extra, p.diag_extra = _p(rhs_extra), _p(diag_extra)
        p.X_out, p.bias_out, p.gram_out, p.factor_out = _p(X_out), _p(bias_out), _p(gram_out), _p(factor_out)
        p.rhs_out, p.colsum_out, p.sumr_out, p.status = _p(rhs_out), _p(colsum_out), _p(sumr_out), _p(status)
        p.sumr2_out, p.stat_out = _p(sumr2_out), _p(stat_out)
        p.tasks, p.ntasks = _p(tasks.tasks), tasks.ntasks
        p.ndual_tail = int(tasks.ndual)      # honoured by the library for plain solves
        p.ndual_mid = int(tasks.nmid)
        p.long_rows, p.nlong = _p(tasks.long_rows), tasks.nlong
        p.workspace = _p(workspace)
        p.F_scale, p.F_scale_ready = _p(self._fscale), 0
        # pre-split operands (als_row_solve_params::F_planes): k = 49 ... 64, f16x2 Gram, a gathered table small enough
        # that the extra pass over it is noise - in practice the U-step (its table is V / Z); the V-step's table (U) is
        # large and that launch is bound by the gather, not by vector issue
        # (the zero row is the table's last row - right behind the view the engine passes as F)
        # k = 113 ... 128: the kernel has the path too (tested), but it measures +-0 there - 124 instead of 108 matrix
        # instructions per 32 ratings cost what the vector instructions save (cfg 5 / 50: V-step 1.93 -> 1.89 ms,
        # U-step unchanged) - so it is off unless ALS_PLANES_K128=1
        nwords = (int(zero_row) + 1) * ld
        limit = self.planes_max_floats if ld == 64 else (self.planes_max_floats_k128 if ld == 128 else 0)
        if (not f64 and p.gram_mode == self.GRAM_MODES["f16x2"] and 0 < nwords <= limit
                and int(zero_row) >= F.shape[0] - 1 and F.is_contiguous()):
            buf = self._planes.get(nwords)
            if buf is None:
                buf = self._planes[nwords] = torch.empty(nwords, dtype=torch.int32, device=self.device)
            p.F_planes = _p(buf)
            p.R_scale = float(residual_scale)
        if self.cond_limit > 0.0 and not self.ablate and not f64:
            if side.nrows not in self._redo_rows:
                self._redo_rows[side.nrows] = torch.empty(max(side.nrows, 1), dtype=torch.int32, device=self.device)
            p.cond_limit = self.cond_limit
            p.redo_count, p.redo_rows = _p(self._redo_count), _p(self._redo_rows[side.nrows])
            p.cond_out = _p(self.cond_probe) if (self.cond_probe is not None and self.cond_probe.numel() >= side.nrows) else None
            if self.solve_dtype == "refine":
                if side.nrows not in self._fallback_rows:
                    self._fallback_rows[side.nrows] = torch.empty(max(side.nrows, 1), dtype=torch.int32, device=self.device)
                r = _hip.RefineParams()
                r.max_steps = int(self.refine_max_steps)
                r.fallback_count, r.fallback_rows = _p(self._fallback_count), _p(self._fallback_rows[side.nrows])
                r.step_hist = _p(self._refine_steps)
                self._check(self.lib.als_row_solve_refine(C.byref(p), C.byref(r), self._stream()), "als_row_solve_refine")
                return
        self._check(self.lib.als_row_solve(C.byref(p), self._stream()), "als_row_solve")

    # -- K2 ------------------------------------------------------------------
    def gs_level(self, *, items, **kw):
        """One dependency level of the sweep (als_gs_sweep); `kw` as `_gs_params` reads it."""
        p = self._gs_params(items, kw)
        self._check(self.lib.als_gs_sweep(C.byref(p), self._stream()), "als_gs_sweep")

    def _gs_params(self, items, kw):
        p = _hip.GsSweepParams()
        p.k, p.ld = kw["k"], kw["ld"]
        p.items, p.nitems = _p(items), items.numel()
        p.S_ptr, p.S_idx, p.S_val, p.alpha = _p(kw["S_ptr"]), _p(kw["S_idx"]), _p(kw["S_val"]), float(kw["alpha"])
        p.factor, p.rhs, p.colsum, p.sumr = _p(kw["factor"]), _p(kw["rhs"]), _p(kw["colsum"]), _p(kw["sumr"])
        p.indptr, p.lambda_bias_scalar, p.lambda_bias_row = _p(kw["indptr"]), float(kw["lam_b"]), _p(kw["lam_b_row"])
        p.V, p.bias = _p(kw["V"]), _p(kw["bias"])
        p.sumr2, p.lambda_eff, p.stat_out = _p(kw.get("sumr2")), _p(kw.get("lambda_eff")), _p(kw.get("stat_out"))
        p.f64 = int(bool(kw.get("f64", False)))
        return p

    def gs_dataflow(self, *, items, S_idx_wait, publish, err, nondep=None, **kw):
        """Whole sweep as one persistent launch; see als_gs_sweep_dataflow."""
        p = self._gs_params(items, kw)
        assert publish.shape == kw["V"].shape and publish.is_contiguous()
        assert nondep is None or (nondep.shape == kw["V"].shape and nondep.is_contiguous())
        self._check(self.lib.als_gs_sweep_dataflow(C.byref(p), _p(S_idx_wait), _p(publish), publish.shape[0], _p(nondep),
                                                   _p(err), self._stream()), "als_gs_sweep_dataflow")

    def gs_levels(self, *, offsets, **kw):
        """All levels of the sweep with one C call (offsets: host int64 numpy array, nlevels+1)."""
        p = self._gs_params(kw.pop("items"), kw)
        p.nitems = 0
        off = offsets.ctypes.data_as(C.c_void_p)
        self._check(self.lib.als_gs_sweep_levels(C.byref(p), off, len(offsets) - 1, self._stream()),
                    "als_gs_sweep_levels")

    # -- K3/K4 ---------------------------------------------------------------
    def w_item_vectors(self, *, k, ld, item_begin, item_end, gram, rhs, colsum, V, b_new, b_old, X, feat_off,
                       W, H, f64=False):
        """`f64`: gram / rhs / colsum / H are double tensors and W is the fp64 projection matrix [D, k]."""
        p = _hip.WParams()
        p.f64 = int(bool(f64))
        p.k, p.ld, p.phase, p.nfeat = k, ld, 0, feat_off.numel() - 1
        p.item_begin, p.item_end = int(item_begin), int(item_end)
        p.gram, p.rhs, p.colsum, p.V, p.b_new, p.b_old = _p(gram), _p(rhs), _p(colsum), _p(V), _p(b_new), _p(b_old)
        p.D, p.X, p.feat_off, p.W, p.H, p.nrows_h = X.shape[1], _p(X), _p(feat_off), _p(W), _p(H), H.shape[1]
        self._check(self.lib.als_w_normal_equations(C.byref(p), self._stream()), "als_w_normal_equations(0)")

    def w_accumulate(self, *, k, ld, item_begin, item_end, gram, X, H, feat_index, feat_col0, feat_d, f64=False):
        """(A [(d k)^2], B [d k]) fp64, storage order, for one feature over items [item_begin, item_end)."""
        npairs = feat_d * (feat_d + 1) // 2
        nit = max(int(item_end) - int(item_begin), 1)
        nchunks = max(1, min(512, 4096 // npairs, -(-nit // 64)))
        kb = ld // 16
        dbl = torch.float64
        partA = torch.empty(npairs * nchunks * (kb * (kb + 1) // 2) * 256, dtype=dbl, device=self.device)
        partB = torch.empty(feat_d * nchunks * ld, dtype=dbl, device=self.device)
        A = torch.empty(feat_d * k, feat_d * k, dtype=dbl, device=self.device)
        B = torch.empty(feat_d * k, dtype=dbl, device=self.device)
        p = _hip.WParams()
        p.f64 = int(bool(f64))
        p.k, p.ld, p.phase = k, ld, 1
        p.item_begin, p.item_end = int(item_begin), int(item_end)
        p.gram, p.D, p.X, p.H, p.nrows_h = _p(gram), X.shape[1], _p(X), _p(H), H.shape[1]
        p.feat_index, p.feat_col0, p.feat_d, p.nchunks = feat_index, feat_col0, feat_d, nchunks
        p.partA, p.partB, p.A_out, p.B_out = _p(partA), _p(partB), _p(A), _p(B)
        self._check(self.lib.als_w_normal_equations(C.byref(p), self._stream()), "als_w_normal_equations(1)")
        return A, B

    def spd_solve(self, A: torch.Tensor, b: torch.Tensor, diag_add: float, status: torch.Tensor) -> torch.Tensor:
        """x = (A + diag_add I)^-1 b, dense fp64 Cholesky (scripts/als.py:497-500).  status: device int32[1]."""
        N = A.shape[0]
        assert A.dtype == torch.float64 and A.is_contiguous() and A.shape == (N, N) and b.numel() == N
        nbytes = int(self.lib.als_spd_solve_workspace_bytes(N))
        if nbytes == 0:
            raise ValueError(f"W-step system of order {N} exceeds ALS_SPD_MAX_N")
        x = torch.empty(N, dtype=torch.float64, device=self.device)
        self._check(self.lib.als_spd_solve_f64(N, _p(A), N, _p(b), float(diag_add), _p(x),
                                               self._workspace("spd", nbytes), _p(status), self._stream()),
                    "als_spd_solve_f64")
        return x

    # -- K6 ------------------------------------------------------------------
    def residual_stats(self, *, k, ld, side, U, Z, b_u, b_i, mu, tasks, out):
        if tasks.ntasks == 0:
            out.zero_()
            return
        need = 2 * ((tasks.ntasks + 3) // 4)
        if self._stats_partials is None or self._stats_partials.numel() < need:
            self._stats_partials = torch.empty(need, dtype=torch.float64, device=self.device)
        self._check(self.lib.als_residual_stats(
            k, ld, _p(side.indptr), _p(side.indices), _p(side.vals), _p(U), _p(Z), _p(b_u), _p(b_i),
            _p(mu), _p(tasks.tasks), tasks.ntasks, _p(self._stats_partials), _p(out), self._stream()),
            "als_residual_stats")

    def item_stats(self, *, k, ld, item_begin, item_end, gram, rhs, colsum, sumr, sumr2, indptr, Z, b_new, b_old,
                   stat_out, f64=False):
        """Per-item closed-form residual sums when Z != V (als_item_stats / als_item_stats_f64)."""
        fn = self.lib.als_item_stats_f64 if f64 else self.lib.als_item_stats
        self._check(fn(k, ld, int(item_begin), int(item_end), _p(gram), _p(rhs), _p(colsum),
                       _p(sumr), _p(sumr2), _p(indptr), _p(Z), _p(b_new), _p(b_old),
                       _p(stat_out), self._stream()), "als_item_stats")

    def sum_pairs(self, x: torch.Tensor, out: torch.Tensor):
        """out[0:2] = column sums of x viewed as [n, 2] (fp64, deterministic)."""
        x = getattr(x, "base", x)           # a rank-local by-product array (containers._RowShift): reduce what exists
        if getattr(self, "_pair_partials", None) is None:
            self._pair_partials = torch.empty(2 * self._sumsq_partials.numel(), dtype=torch.float64, device=self.device)
        part = self._pair_partials
        self._check(self.lib.als_sum_pairs(_p(x), x.numel() // 2, _p(part), _p(out), self._stream()),
                    "als_sum_pairs")

    def history_row(self, *, U, V, b_u, b_i, stats, nnz, mu, row):
        """mu update + the five history values of an iteration in two launches (als_history_row)."""
        if getattr(self, "_hist_partials", None) is None:
            self._hist_partials = torch.empty(4 * self._sumsq_partials.numel(), dtype=torch.float64, device=self.device)
        self._check(self.lib.als_history_row(_p(U), U.numel(), _p(V), V.numel(), _p(b_u), b_u.numel(), _p(b_i), b_i.numel(),
                                             _p(stats), int(nnz), _p(mu), _p(self._hist_partials), _p(row), self._stream()),
                    "als_history_row")

    def sumsq(self, x: torch.Tensor, out: torch.Tensor):
        self._check(self.lib.als_sumsq(_p(x), x.numel(), _p(self._sumsq_partials), _p(out),
                                       self._stream()), "als_sumsq")

    # -- K0 / K7 ---------------------------------------------------------------
    def compose_z(self, V, X, W, Z):
        D = 0 if X is None else X.shape[1]
        self._check(self.lib.als_compose_z(V.shape[0], V.shape[1], D, _p(V), _p(X), _p(W), _p(Z),
                                           self._stream()), "als_compose_z")

    def predict_at(self, *, k, ld, us, is_, U, Z, b_u, b_i, mu, out):
        self._check(self.lib.als_predict_at(k, ld, us.numel(), _p(us), _p(is_), _p(U), _p(Z), _p(b_u),
                                            _p(b_i), _p(mu), _p(out), self._stream()), "als_predict_at")

    def predict_dense(self, *, k, ld, m, n, U, Z, b_u, b_i, mu, out):
        self._check(self.lib.als_predict_dense(k, ld, m, n, _p(U), _p(Z), _p(b_u), _p(b_i), _p(mu),
                                               _p(out), self._stream()), "als_predict_dense")

    @staticmethod
    def recommend_slices() -> int:
        # item slices of als_recommend_topk: 0 = automatic; ALS_RECOMMEND_SLICES forces a count (tests: the result
        # must not depend on it)
        return int(os.environ.get("ALS_RECOMMEND_SLICES", "0"))

    def recommend_topk(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, top_val, top_idx,
                       top_cnt):
        """Top-`topn` items of every user in `users` (int32), seen items (CSR by user id; None = none) left out:
        als_recommend_topk.  The item-slice workspace is owned here and grows as needed."""
        self._recommend(self.lib.als_recommend_topk, "als_recommend_topk", (), k, ld, users, n, U, Z, b_u, b_i, mu,
                        seen_ptr, seen_idx, topn, top_val, top_idx, top_cnt)

    def recommend_topk_masked(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, topn, top_val,
                              top_idx, top_cnt):
        """`recommend_topk` over the items of the bitmap `allow` (int32 [ceil(n / 32)], item i = bit i & 31 of word
        i >> 5): als_recommend_topk_masked."""
        if allow is None:
            raise ValueError("recommend_topk_masked needs an allow bitmap; recommend_topk is the call without one")
        self._recommend(self.lib.als_recommend_topk_masked, "als_recommend_topk_masked", (self._bitmap(allow, n),), k,
                        ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, top_val, top_idx, top_cnt)

    def _recommend(self, fn, what, allow, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, top_val,
                   top_idx, top_cnt):
        # the empty-seen rule and the workspace are written out here and in `_rank`, not taken from `_seen` /
        # `_workspace`: these two serve the small-batch calls, where two more Python calls per call showed
        if seen_idx is not None and seen_idx.numel() == 0:      # every row empty (and no storage to point at)
            seen_ptr = seen_idx = None
        nsl = self.recommend_slices()
        need = int(self.lib.als_recommend_workspace_bytes(users.numel(), n, topn, nsl))
        if need > 0 and (self._rec_ws is None or self._rec_ws.numel() < need):
            self._rec_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._check(fn(k, ld, users.numel(), _p(users), n, _p(U), _p(Z), _p(b_u), _p(b_i), _p(mu), _p(seen_ptr),
                       _p(seen_idx), *allow, topn, nsl, _p(top_val), _p(top_idx), _p(top_cnt),
                       _p(self._rec_ws) if need > 0 else None, need, self._stream()), what)

    def recommend_deep(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, after_key, topn,
                       top_val, top_idx, top_cnt, rounds=None):
        """`recommend_topk_masked` (allow None: every item) for topn up to ALS_TOPK_DEEP_MAX = 1024, optionally below
        a cursor: als_recommend_deep.  after_key: None, or int64 [B] holding the bits of the 64-bit cursor keys
        (serving.cursor_keys); rounds: None or an int32 [1] device tensor that receives the scoring rounds that did work.
        The workspace is owned here and grows as needed; ALS_RECOMMEND_SLICES applies."""
        allow = self._bitmap(allow, n)
        if after_key is not None and (after_key.dtype != torch.int64 or not after_key.is_cuda
                                      or not after_key.is_contiguous() or after_key.numel() != users.numel()):
            raise ValueError("after_key must be a contiguous int64 device tensor with one key per batch row")
        need = self.recommend_deep_workspace_bytes(users.numel(), n, topn)
        self._check(self.lib.als_recommend_deep(
            k, ld, users.numel(), _p(users), n, _p(U), _p(Z), _p(b_u), _p(b_i), _p(mu), *self._seen(seen_ptr, seen_idx),
            allow, _p(after_key), topn, self.recommend_slices(), _p(top_val), _p(top_idx), _p(top_cnt), _p(rounds),
            self._workspace("recommend_deep", need), need, self._stream()), "als_recommend_deep")

    def recommend_deep_workspace_bytes(self, nusers: int, n: int, topn: int) -> int:
        """Bytes of workspace a `recommend_deep` call over `nusers` rows takes (als_recommend_deep_workspace_bytes
        under the slice count in force)."""
        return int(self.lib.als_recommend_deep_workspace_bytes(nusers, n, topn, self.recommend_slices()))

    def rank_count(self, *, k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, q_users, q_ptr, q_items, t_score,
                   above, n_cand):
        """For every target of every batch row (user q_users[b], targets q_items[q_ptr[b]:q_ptr[b+1]]) the score
        and the number of unseen items ranked above it, and per row the number of candidates: als_rank_count.
        The item-slice workspace is owned here and grows as needed; ALS_RECOMMEND_SLICES applies."""
        self._rank(self.lib.als_rank_count, "als_rank_count", (), k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx,
                   q_users, q_ptr, q_items, t_score, above, n_cand)

    def rank_count_masked(self, *, k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, q_users, q_ptr, q_items,
                          t_score, above, n_cand):
        """`rank_count` with the candidates limited to the bitmap `allow` (as `recommend_topk_masked`):
        als_rank_count_masked."""
        if allow is None:
            raise ValueError("rank_count_masked needs an allow bitmap; rank_count is the call without one")
        self._rank(self.lib.als_rank_count_masked, "als_rank_count_masked", (self._bitmap(allow, n),), k, ld, n, U, Z,
                   b_u, b_i, mu, seen_ptr, seen_idx, q_users, q_ptr, q_items, t_score, above, n_cand)

    def _segment_args(self, seg_allow: torch.Tensor, row_seg: torch.Tensor, n: int, rows: int):
        # the kernels index the table by (segment, item word) and row_seg by batch row: anything short is an
        # out-of-bounds read.  Ids outside [0, S) are the kernel's to refuse (such a row gets no candidates)
        W = (n + 31) // 32
        if (seg_allow.dtype != torch.int32 or not seg_allow.is_cuda or not seg_allow.is_contiguous()
                or seg_allow.dim() != 2 or seg_allow.shape[0] < 1 or seg_allow.shape[1] < W):
            raise ValueError(f"eligibility table must be a contiguous int32 device tensor [S >= 1, >= {W} words]")
        if (row_seg.dtype != torch.int32 or not row_seg.is_cuda or not row_seg.is_contiguous()
                or row_seg.numel() != rows):
            raise ValueError("row_seg must be a contiguous int32 device tensor with one segment id per batch row")
        return _p(seg_allow), seg_allow.shape[0], seg_allow.shape[1], _p(row_seg)

    def recommend_topk_segmented(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, seg_allow, row_seg,
                                 topn, top_val, top_idx, top_cnt):
        """`recommend_topk_masked` with the bitmap of batch row b being row row_seg[b] (int32 [B]) of the table
        `seg_allow` (int32 [S, >= ceil(n / 32)]): als_recommend_topk_segmented."""
        seg = self._segment_args(seg_allow, row_seg, n, users.numel())
        self._recommend(self.lib.als_recommend_topk_segmented, "als_recommend_topk_segmented", seg, k, ld, users, n, U,
                        Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, top_val, top_idx, top_cnt)

    def rank_count_segmented(self, *, k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, seg_allow, row_seg, q_users,
                             q_ptr, q_items, t_score, above, n_cand):
        """`rank_count_masked` with one table row per batch row, as `recommend_topk_segmented`:
        als_rank_count_segmented."""
        seg = self._segment_args(seg_allow, row_seg, n, q_users.numel())
        self._rank(self.lib.als_rank_count_segmented, "als_rank_count_segmented", seg, k, ld, n, U, Z, b_u, b_i, mu,
                   seen_ptr, seen_idx, q_users, q_ptr, q_items, t_score, above, n_cand)

    def eligibility_bitmaps(self, *, n, item_tags, need_all, need_any, forbid, base_allow, out):
        """out int32 [S, ceil(n / 32)] = the eligibility table of the rules need_all / need_any / forbid (int32 [S, tw]
        each, None = all zero) over item_tags (int32 [n, tw]), ANDed with the bitmap base_allow (or None):
        als_eligibility_bitmaps."""
        tw, S = item_tags.shape[1], out.shape[0]
        assert item_tags.dtype == torch.int32 and item_tags.is_contiguous() and item_tags.shape[0] == n
        assert out.dtype == torch.int32 and out.is_contiguous() and out.shape[1] == (n + 31) // 32
        for r in (need_all, need_any, forbid):
            assert r is None or (r.dtype == torch.int32 and r.is_contiguous() and tuple(r.shape) == (S, tw))
        self._check(self.lib.als_eligibility_bitmaps(n, tw, _p(item_tags), S, _p(need_all), _p(need_any), _p(forbid),
                                                     self._bitmap(base_allow, n), _p(out), self._stream()),
                    "als_eligibility_bitmaps")

    @staticmethod
    def _keys(t: torch.Tensor, n: int, what: str):
        """Pointer to n 64-bit keys carried as int64 bit patterns (as `recommend_deep` carries after_key), checked."""
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"{what} must be a contiguous int64 device tensor of {n} keys")
        return _p(t)

    def recommend_topk_priced(self, *, k, ld, users, row_ids, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow,
                              floor_key, topn, top_val, top_idx, top_cnt):
        """`recommend_topk_masked` (allow None: every item) where launched row b takes item i only if its item-side key
        make_key(score, row_ids[b]) is >= floor_key[i]: als_recommend_topk_priced.  row_ids int32 [B]: the batch row of
        every launched row; floor_key int64 [n]: the bits of the 64-bit floors."""
        if row_ids.dtype != torch.int32 or not row_ids.is_cuda or not row_ids.is_contiguous() \
                or row_ids.numel() != users.numel():
            raise ValueError("row_ids must be a contiguous int32 device tensor with one batch row per launched row")
        self._recommend(self.lib.als_recommend_topk_priced, "als_recommend_topk_priced",
                        (self._bitmap(allow, n), _p(row_ids), self._keys(floor_key, n, "floor_key")), k, ld, users, n,
                        U, Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, top_val, top_idx, top_cnt)

    def capacity_settle(self, *, n, top_idx, top_val, capacity, floor_key, fill, dirty, n_over):
        """From the whole batch's lists (top_idx int32 / top_val fp32 [B, topn]) and capacity int32 [n]: fill int32 [n] =
        min(demand, capacity), the floors (int64 [n], in / out) of the over-demanded items raised to their
        capacity-th largest item-side key, dirty int32 [B] = the row holds an item it no longer passes, n_over int32 [1]
        = the over-demanded items: als_capacity_settle.  No host synchronisation; the workspace is owned here."""
        B, topn = top_idx.shape
        for t, dt, num in ((top_idx, torch.int32, B * topn), (top_val, torch.float32, B * topn),
                           (capacity, torch.int32, n), (fill, torch.int32, n), (dirty, torch.int32, B),
                           (n_over, torch.int32, 1)):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous() or t.numel() != num:
                raise ValueError("capacity_settle: the lists, capacity, fill, dirty and n_over must be contiguous device "
                                 "tensors of their documented dtypes and sizes")
        need = int(self.lib.als_capacity_settle_workspace_bytes(B, n, topn))
        if need == 0:
            raise ValueError("capacity_settle: B * topn and n must be below 2^31")
        self._check(self.lib.als_capacity_settle(B, topn, n, _p(top_idx), _p(top_val), _p(capacity),
                                                 self._keys(floor_key, n, "floor_key"), _p(fill), _p(dirty), _p(n_over),
                                                 self._workspace("capacity_settle", need), need, self._stream()),
                    "als_capacity_settle")

    def recommend_topk_quota(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, item_group,
                             group_cap, topn, top_val, top_idx, top_cnt):
        """`recommend_topk_masked` (allow None: every item) with at most group_cap[g] items of group g in a list:
        als_recommend_topk_quota.  item_group int32 [n]: the label of every item (outside [0, G): no group);
        group_cap int32 [G]."""
        for t, num, what in ((item_group, n, "item_group"), (group_cap, group_cap.numel(), "group_cap")):
            if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous() or t.numel() != num:
                raise ValueError(f"{what} must be a contiguous int32 device tensor"
                                 + (f" of {n} labels" if what == "item_group" else ""))
        self._recommend(self.lib.als_recommend_topk_quota, "als_recommend_topk_quota",
                        (self._bitmap(allow, n), _p(item_group), _p(group_cap) if group_cap.numel() else None,
                         group_cap.numel()), k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, top_val,
                        top_idx, top_cnt)

    def _rank(self, fn, what, allow, k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, q_users, q_ptr, q_items,
              t_score, above, n_cand):
        if seen_idx is not None and seen_idx.numel() == 0:
            seen_ptr = seen_idx = None
        nq, nt = q_users.numel(), q_items.numel()
        nsl = self.recommend_slices()
        need = int(self.lib.als_rank_count_workspace_bytes(k, nq, nt, n, nsl))
        if need > 0 and (self._rank_ws is None or self._rank_ws.numel() < need):
            self._rank_ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._check(fn(k, ld, n, _p(U), _p(Z), _p(b_u), _p(b_i), _p(mu), _p(seen_ptr), _p(seen_idx), *allow, nq,
                       _p(q_users), _p(q_ptr), _p(q_items) if nt else None, nt, nsl, _p(t_score) if nt else None,
                       _p(above) if nt else None, _p(n_cand), _p(self._rank_ws) if need > 0 else None, need,
                       self._stream()), what)

    # -- K9 --------------------------------------------------------------------
    def fold_in(self, *, k, ld, indptr, indices, vals, n, Z, b_i, mu, lam_u, lam_bu, n_sweeps, U_out, b_u_out,
                status):
        """Factors / biases of the rows of a CSR (device: int64 indptr, int32 indices, fp32 vals) against the fixed
        item side: als_fold_in.  n_sweeps 0 = fixed point."""
        p = _hip.FoldInParams()
        p.k, p.ld, p.nrows, p.n_sweeps = k, ld, indptr.numel() - 1, int(n_sweeps)
        p.indptr, p.indices, p.vals = _p(indptr), _p(indices), _p(vals)
        p.n, p.Z, p.b_i, p.mu = int(n), _p(Z), _p(b_i), _p(mu)
        p.lambda_u, p.lambda_bu = float(lam_u), float(lam_bu)
        p.U_out, p.b_u_out, p.status = _p(U_out), _p(b_u_out), _p(status)
        self._check(self.lib.als_fold_in(C.byref(p), self._stream()), "als_fold_in")

    def fold_in_items(self, *, k, ld, indptr, indices, vals, m, U, b_u, mu, S, n, V, lam_v, pop_reg, lam_bi, alpha,
                      n_sweeps, V_out, b_i_out, status):
        """Factors / biases of new items (ratings CSR by rater id; device: int64 indptr, int32 indices, fp32 vals)
        against the fixed user side and the fitted V, with graph rows S = (ptr, idx, val) or None:
        als_fold_in_items.  n_sweeps 0 = fixed point."""
        p = _hip.FoldInItemsParams()
        p.k, p.ld, p.nrows, p.n_sweeps, p.pop_reg = k, ld, indptr.numel() - 1, int(n_sweeps), int(bool(pop_reg))
        p.indptr, p.indices, p.vals = _p(indptr), _p(indices), _p(vals)
        p.m, p.U, p.b_u, p.mu = int(m), _p(U), _p(b_u), _p(mu)
        if S is not None:
            p.S_ptr, p.S_idx, p.S_val = _p(S[0]), _p(S[1]), _p(S[2])
        p.n, p.V = int(n), _p(V)
        p.lambda_v, p.lambda_bi, p.alpha = float(lam_v), float(lam_bi), float(alpha)
        p.V_out, p.b_i_out, p.status = _p(V_out), _p(b_i_out), _p(status)
        self._check(self.lib.als_fold_in_items(C.byref(p), self._stream()), "als_fold_in_items")

    # -- K18 -------------------------------------------------------------------
    def table_gram_doubles(self, ld: int) -> int:
        """Doubles of one Gram image of als_table_gram_f64: the lower 16 x 16 blocks of an ld x ld matrix."""
        kb = ld // 16
        return kb * (kb + 1) // 2 * 256

    def table_gram(self, k, ld, F, out, w=None):
        """out fp64 [table_gram_doubles(ld)] = F^T F over all rows of the fp32 table F [rows, ld], the perm-space
        lower-block image als_implicit_row_solve takes: als_table_gram_f64.  With the row weights w (fp32 [rows]):
        F^T diag(w) F, als_table_gram_weighted_f64.  The partials are owned here."""
        assert F.dtype == torch.float32 and F.is_contiguous() and F.shape[1] == ld
        assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= self.table_gram_doubles(ld)
        need = 8 * int(self.lib.als_table_gram_partials()) * self.table_gram_doubles(ld)
        if w is None:
            self._check(self.lib.als_table_gram_f64(k, ld, F.shape[0], _p(F), self._workspace("table_gram", need),
                                                    _p(out), self._stream()), "als_table_gram_f64")
            return
        assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() >= F.shape[0] and w.device == F.device
        self._check(self.lib.als_table_gram_weighted_f64(k, ld, F.shape[0], _p(F), _p(w),
                                                         self._workspace("table_gram", need), _p(out),
                                                         self._stream()), "als_table_gram_weighted_f64")

    def implicit_row_solve(self, *, k, ld, side, F, zero_row, G, g_scale, lam, lam_row, X_out, xb_out, status, tasks,
                           rhs_w=None, g_scale_row=None):
        """x = (g_scale G + sum a f f^T + (lam + 1e-10) I)^-1 sum t f for the rows of `tasks` (side.vals holds the
        weights a; rhs_w the t, None: t = 1 + a); rows of `side` without entries get x = 0: als_implicit_row_solve.
        g_scale_row (fp32 [side.nrows]): row r takes g_scale g_scale_row[r] in place of g_scale.
        zero_row: the row of F that lanes past a row's end gather, or -1.  The slot workspace is owned here."""
        if g_scale_row is not None:
            assert (g_scale_row.dtype == torch.float32 and g_scale_row.is_contiguous()
                    and g_scale_row.numel() >= side.nrows and g_scale_row.device == F.device)
        p = _hip.ImplicitParams()
        p.k, p.ld, p.nrows, p.ncols, p.F_zero_row = k, ld, side.nrows, F.shape[0], int(zero_row)
        assert F.dtype == torch.float32 and F.is_contiguous() and F.shape[1] == ld and -1 <= int(zero_row) < F.shape[0]
        assert X_out.is_contiguous() and X_out.shape[0] >= side.nrows and X_out.shape[1] == ld
        assert G.dtype == torch.float64 and G.numel() >= self.table_gram_doubles(ld)
        p.indptr, p.indices, p.gram_w, p.rhs_w = _p(side.indptr), _p(side.indices), _p(side.vals), _p(rhs_w)
        p.F, p.G, p.G_scale = _p(F), _p(G), float(g_scale)
        p.lambda_scalar, p.lambda_row = float(lam), _p(lam_row)
        p.X_out, p.xb_out, p.status = _p(X_out), _p(xb_out), _p(status)
        p.tasks, p.ntasks = _p(tasks.tasks), tasks.ntasks
        p.long_rows, p.nlong = _p(tasks.long_rows), tasks.nlong
        p.workspace = self._workspace("implicit_slots", tasks.nslots * self.slot_bytes(k, True))
        p.g_scale_row = _p(g_scale_row)
        self._check(self.lib.als_implicit_row_solve(C.byref(p), self._stream()), "als_implicit_row_solve")

    # -- K11 -------------------------------------------------------------------
    def explain(self, *, k, ld, indptr, indices, vals, rows, n, Z, b_i, mu, lam_u, lam_bu, n_sweeps, t_ptr, t_items,
                topm, largest, score, latent, leverage, top_item, top_contrib, top_weight, top_cnt, b_u_out, status):
        """Per target of every work row (work row w reads CSR row rows[w], or row w when `rows` is None; targets
        t_items[t_ptr[w]:t_ptr[w+1]]) the score, its latent part, the leverage and the `topm` strongest
        contributions of the row's ratings: als_explain.  n_sweeps 0 = fixed point."""
        p = _hip.ExplainParams()
        p.k, p.ld, p.nrows, p.n_sweeps = k, ld, t_ptr.numel() - 1, int(n_sweeps)
        p.topm, p.largest = int(topm), int(bool(largest))
        p.indptr, p.indices, p.vals, p.rows = _p(indptr), _p(indices), _p(vals), _p(rows)
        p.n, p.Z, p.b_i, p.mu = int(n), _p(Z), _p(b_i), _p(mu)
        p.lambda_u, p.lambda_bu = float(lam_u), float(lam_bu)
        p.t_ptr, p.t_items = _p(t_ptr), _p(t_items)
        p.score, p.latent, p.leverage = _p(score), _p(latent), _p(leverage)
        p.top_item, p.top_contrib, p.top_weight, p.top_cnt = _p(top_item), _p(top_contrib), _p(top_weight), _p(top_cnt)
        p.b_u_out, p.status = _p(b_u_out), _p(status)
        self._check(self.lib.als_explain(C.byref(p), self._stream()), "als_explain")

    # -- K12 -------------------------------------------------------------------
    def mmr_rerank(self, *, k, ld, n, Z, cand_val, cand_idx, lam, topn, top_val, top_idx, top_cnt, top_ild=None):
        """Greedy MMR re-ranking of the pools cand_val fp32 / cand_idx int32 [B, pool] (the outputs of
        `recommend_topk` with topn = pool) against Z: top_val / top_idx [B, topn], top_cnt [B], top_ild fp32 [B] or
        None: als_mmr_rerank."""
        B, pool = cand_idx.shape
        assert cand_val.shape == (B, pool) and cand_val.is_contiguous() and cand_idx.is_contiguous()
        self._check(self.lib.als_mmr_rerank(k, ld, B, n, _p(Z), pool, _p(cand_val), _p(cand_idx), float(lam), topn,
                                            _p(top_val), _p(top_idx), _p(top_cnt), _p(top_ild), self._stream()),
                    "als_mmr_rerank")

    def list_diversity(self, *, k, ld, n, Z, idx, ild):
        """ild fp32 [B] = intra-list diversity of the id lists idx int32 [B, L] (-1 padded): als_list_diversity."""
        B, L = idx.shape
        assert idx.is_contiguous()
        self._check(self.lib.als_list_diversity(k, ld, B, n, _p(Z), L, _p(idx), _p(ild), self._stream()),
                    "als_list_diversity")

    # -- K13 -------------------------------------------------------------------
    def row_inv_norms(self, *, k, ld, T, inv_norm):
        """inv_norm fp32 [rows] = 1 / |T_r| of the rows of T fp32 [rows, ld], squares summed in fp64; 0 for a zero
        row, NaN for a row with a non-finite entry: als_row_inv_norms."""
        assert T.is_contiguous() and T.shape[1] == ld and inv_norm.numel() >= T.shape[0]
        self._check(self.lib.als_row_inv_norms(k, ld, T.shape[0], _p(T), _p(inv_norm), self._stream()),
                    "als_row_inv_norms")

    def similar_topk(self, *, k, ld, q_ids, Q, q_inv, self_ids, n, T, t_inv, allow, topn, top_val, top_idx, top_cnt):
        """Top-`topn` rows of T [n, ld] by cosine for every query row q_ids[b] (int32) of Q, row self_ids[b] left
        out (None: no exclusion), restricted to the bitmap `allow` (None: every row); q_inv / t_inv are the
        `row_inv_norms` of Q / T: als_similar_topk.  The slice workspace is owned here and grows as needed;
        ALS_RECOMMEND_SLICES applies."""
        allow = self._bitmap(allow, n)
        nq = q_ids.numel()
        nsl = self.recommend_slices()
        need = int(self.lib.als_similar_workspace_bytes(nq, n, topn, nsl))
        self._check(self.lib.als_similar_topk(k, ld, nq, _p(q_ids), _p(Q), _p(q_inv), _p(self_ids), n, _p(T),
                                              _p(t_inv), allow, topn, nsl, _p(top_val), _p(top_idx), _p(top_cnt),
                                              self._workspace("similar", need), need, self._stream()),
                    "als_similar_topk")

    # -- K14 -------------------------------------------------------------------
    def audience_topk(self, *, k, ld, q_ids, Q, q_bias, m, U, b_u, mu, seen_ptr, seen_idx, allow, topn, top_val,
                      top_idx, top_cnt):
        """Top-`topn` users of every query item q_ids[b] (int32, a row of Q / q_bias), the item's raters (CSR by
        ITEM id over user ids; None = none) left out, restricted to the user bitmap `allow` (None: every user):
        als_audience_topk.  The slice workspace is owned here and grows as needed; ALS_RECOMMEND_SLICES applies."""
        allow = self._bitmap(allow, m)
        nq = q_ids.numel()
        nsl = self.recommend_slices()
        need = int(self.lib.als_audience_workspace_bytes(nq, m, topn, nsl))
        self._check(self.lib.als_audience_topk(k, ld, nq, _p(q_ids), _p(Q), _p(q_bias), m, _p(U), _p(b_u), _p(mu),
                                               *self._seen(seen_ptr, seen_idx), allow, topn, nsl, _p(top_val),
                                               _p(top_idx), _p(top_cnt), self._workspace("audience", need), need,
                                               self._stream()), "als_audience_topk")

    # -- K15 -------------------------------------------------------------------
    GROUP_AGGREGATES = {"mean": 0, "min": 1, "max": 2}     # ALS_GROUP_MEAN / _MIN / _MAX

    def group_topk(self, *, k, ld, g_ptr, g_users, max_members, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow,
                   aggregate, topn, top_val, top_idx, top_cnt):
        """Top-`topn` items of every group: group b has the members g_users[g_ptr[b]:g_ptr[b + 1]] (int64 prefix sum,
        int32 rows of U / b_u; at most `max_members` <= 64 each), its score for an item is the `aggregate` ("mean",
        "min", "max") of the members' scores, the items of row b of the seen CSR (indexed by BATCH GROUP; None =
        none) are left out, restricted to the item bitmap `allow` (None: every item): als_group_topk.  The slice
        workspace is owned here and grows as needed; ALS_RECOMMEND_SLICES applies."""
        allow = self._bitmap(allow, n)
        ng = g_ptr.numel() - 1
        nsl = self.recommend_slices()
        need = int(self.lib.als_group_workspace_bytes(ng, n, topn, nsl))
        self._check(self.lib.als_group_topk(k, ld, ng, _p(g_ptr), _p(g_users), int(max_members), n, _p(U), _p(Z),
                                            _p(b_u), _p(b_i), _p(mu), *self._seen(seen_ptr, seen_idx), allow,
                                            self.GROUP_AGGREGATES[aggregate], topn, nsl, _p(top_val), _p(top_idx),
                                            _p(top_cnt), self._workspace("group", need), need, self._stream()),
                    "als_group_topk")

    # -- K16 -------------------------------------------------------------------
    def row_whitener(self, *, k, ld, indptr, indices, rows, n, Z, lam_u, W_out, status):
        """W_out fp32 [rows, ld, ld] = float32(L^-1), L the lower Cholesky factor of Z_S^T Z_S + (lam_u + 1e-10) I
        of every work row (work row w reads CSR row rows[w], or row w when `rows` is None): als_row_whitener."""
        nrows = indptr.numel() - 1 if rows is None else rows.numel()
        assert W_out.is_contiguous() and W_out.shape[1:] == (ld, ld) and W_out.shape[0] >= nrows
        self._check(self.lib.als_row_whitener(k, ld, nrows, _p(indptr), _p(indices), _p(rows), int(n), _p(Z),
                                              float(lam_u), _p(W_out), _p(status), self._stream()),
                    "als_row_whitener")

    def explore_topk(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, W, beta, seen_ptr, seen_idx, allow, topn, top_val,
                     top_idx, top_cnt, top_lev):
        """`recommend_topk_masked` (allow None: every item) with the key score + beta * sqrt(|W_b z_i|^2), W fp32
        [B, ld, ld] by batch row (`row_whitener`); top_lev fp32 [B, topn] receives the leverages of the returned
        items: als_explore_topk.  The slice workspace is owned here and grows as needed; ALS_RECOMMEND_SLICES
        applies."""
        allow = self._bitmap(allow, n)
        B = users.numel()
        assert W.is_contiguous() and W.shape[1:] == (ld, ld) and W.shape[0] >= B
        nsl = self.recommend_slices()
        need = int(self.lib.als_explore_workspace_bytes(k, B, n, topn, nsl))
        self._check(self.lib.als_explore_topk(k, ld, B, _p(users), n, _p(U), _p(Z), _p(b_u), _p(b_i), _p(mu), _p(W),
                                              float(beta), *self._seen(seen_ptr, seen_idx), allow, topn, nsl,
                                              _p(top_val), _p(top_idx), _p(top_cnt), _p(top_lev),
                                              self._workspace("explore", need), need, self._stream()),
                    "als_explore_topk")

    # -- K17 -------------------------------------------------------------------
    def category_profile(self, *, ncat, indptr, indices, rows, n, C, P_out):
        """P_out fp32 [B, ldc] = the mean category row of the categorised items of every batch row's CSR row (batch
        row b reads row rows[b], or row b when `rows` is None; the sum in fp64), all zero without one:
        als_category_profile.  C fp32 [n, ldc] is the category table (validate.category_table)."""
        B = indptr.numel() - 1 if rows is None else rows.numel()
        ldc = C.shape[1]
        assert C.is_contiguous() and C.shape[0] == n and P_out.is_contiguous() and P_out.shape == (B, ldc)
        self._check(self.lib.als_category_profile(ncat, ldc, B, _p(rows), _p(indptr), _p(indices), int(n), _p(C),
                                                  _p(P_out), self._stream()), "als_category_profile")

    def calibrated_rerank(self, *, ncat, n, C, P, cand_val, cand_idx, lam, alpha, topn, top_val, top_idx, top_cnt,
                          top_kl=None):
        """Greedy calibrated re-ranking of the pools cand_val fp32 / cand_idx int32 [B, pool] (the outputs of
        `recommend_topk` with topn = pool) towards the targets P fp32 [B, ldc] over the category table C [n, ldc]:
        top_val / top_idx [B, topn], top_cnt [B], top_kl fp32 [B] or None: als_calibrated_rerank."""
        B, pool = cand_idx.shape
        ldc = C.shape[1]
        assert cand_val.shape == (B, pool) and cand_val.is_contiguous() and cand_idx.is_contiguous()
        assert C.is_contiguous() and C.shape[0] == n and P.is_contiguous() and P.shape == (B, ldc)
        self._check(self.lib.als_calibrated_rerank(ncat, ldc, B, n, _p(C), _p(P), pool, _p(cand_val), _p(cand_idx),
                                                   float(lam), float(alpha), topn, _p(top_val), _p(top_idx),
                                                   _p(top_cnt), _p(top_kl), self._stream()), "als_calibrated_rerank")

    def list_miscalibration(self, *, ncat, n, C, P, idx, alpha, kl):
        """kl fp32 [B] = the smoothed KL divergence of the targets P [B, ldc] from the category distribution of the id
        lists idx int32 [B, L] (-1 padded): als_list_miscalibration."""
        B, L = idx.shape
        ldc = C.shape[1]
        assert idx.is_contiguous() and C.is_contiguous() and C.shape[0] == n and P.is_contiguous() and P.shape == (B, ldc)
        self._check(self.lib.als_list_miscalibration(ncat, ldc, B, n, _p(C), _p(P), L, _p(idx), float(alpha), _p(kl),
                                                     self._stream()), "als_list_miscalibration")
