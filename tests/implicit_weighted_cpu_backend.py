"""TEST-ONLY stand-in for the weighted implicit-feedback entries of `backend.HipBackend`: `ImplicitNumpyBackend` whose
`table_gram` accepts `w=` and whose `implicit_row_solve` accepts `g_scale_row=`, from tests/implicit_weighted_ref.py.
Without the keyword each call is the parent's."""
import numpy as np
import torch

from tests import implicit_ref as iref
from tests import implicit_weighted_ref as wref
from tests.cpu_backend import _np
from tests.implicit_cpu_backend import ImplicitNumpyBackend


class WeightedImplicitNumpyBackend(ImplicitNumpyBackend):
    name = "numpy-test-implicit-weighted"

    def table_gram(self, k, ld, F, out, w=None):
        if w is None:
            return super().table_gram(k, ld, F, out)
        assert w.dtype == torch.float32 and w.numel() >= F.shape[0]
        img = iref.gram_image(wref.table_gram(_np(F)[:, :k], _np(w)[: F.shape[0]]), k)
        out[: img.size] = torch.from_numpy(img)

    def implicit_row_solve(self, *, k, ld, side, F, zero_row, G, g_scale, lam, lam_row, X_out, xb_out, status, tasks,
                           rhs_w=None, g_scale_row=None):
        if g_scale_row is None:
            return super().implicit_row_solve(k=k, ld=ld, side=side, F=F, zero_row=zero_row, G=G, g_scale=g_scale,
                                              lam=lam, lam_row=lam_row, X_out=X_out, xb_out=xb_out, status=status,
                                              tasks=tasks, rhs_w=rhs_w)
        assert g_scale_row.dtype == torch.float32 and g_scale_row.numel() >= side.nrows
        ptr, idx, a = _np(side.indptr), _np(side.indices), _np(side.vals).astype(np.float64)
        t = 1.0 + a if rhs_w is None else _np(rhs_w).astype(np.float64)
        Fn = _np(F)[:, :k].astype(np.float64)
        Gn = iref.gram_from_image(_np(G), k)[0]
        s_row = _np(g_scale_row)
        for r in np.nonzero(np.diff(ptr) == 0)[0]:
            X_out[r] = 0.0
            if xb_out is not None:
                xb_out[r] = 0.0
        for r in self._rows(tasks):
            s = slice(ptr[r], ptr[r + 1])
            try:
                x, b = iref.row_solve(Fn[idx[s]], a[s], t[s], (g_scale * float(s_row[r])) * Gn,
                                      float(lam_row[r]) if lam_row is not None else lam)
            except np.linalg.LinAlgError:
                status[0] = max(int(status[0]), int(r) + 1)
                continue
            xo = np.zeros(ld, dtype=np.float32)
            xo[:k] = x
            X_out[r] = torch.from_numpy(xo)
            if xb_out is not None:
                xb_out[r] = float(x @ b)
