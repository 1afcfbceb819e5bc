"""TEST-ONLY stand-in for the implicit-feedback entries of `backend.HipBackend`: `tests.cpu_backend.NumpyBackend` plus
`table_gram` and `implicit_row_solve` from tests/implicit_ref.py, with the conventions of the C ABI (the Gram as the
perm-space lower-block image, x rounded to fp32, padding columns zero, rows without entries zero)."""
import numpy as np
import torch

from tests import implicit_ref as iref
from tests.cpu_backend import NumpyBackend, _np


class ImplicitNumpyBackend(NumpyBackend):
    name = "numpy-test-implicit"

    def table_gram(self, k, ld, F, out):
        img = iref.gram_image(iref.table_gram(_np(F)[:, :k]), k)
        out[: img.size] = torch.from_numpy(img)

    def implicit_row_solve(self, *, k, ld, side, F, zero_row, G, g_scale, lam, lam_row, X_out, xb_out, status, tasks,
                           rhs_w=None):
        ptr, idx, a = _np(side.indptr), _np(side.indices), _np(side.vals).astype(np.float64)
        t = 1.0 + a if rhs_w is None else _np(rhs_w).astype(np.float64)
        Fn = _np(F)[:, :k].astype(np.float64)
        Gn = g_scale * iref.gram_from_image(_np(G), k)[0]
        for r in np.nonzero(np.diff(ptr) == 0)[0]:
            X_out[r] = 0.0
            if xb_out is not None:
                xb_out[r] = 0.0
        for r in self._rows(tasks):
            s = slice(ptr[r], ptr[r + 1])
            try:
                x, b = iref.row_solve(Fn[idx[s]], a[s], t[s], Gn, float(lam_row[r]) if lam_row is not None else lam)
            except np.linalg.LinAlgError:
                status[0] = max(int(status[0]), int(r) + 1)
                continue
            xo = np.zeros(ld, dtype=np.float32)
            xo[:k] = x
            X_out[r] = torch.from_numpy(xo)
            if xb_out is not None:
                xb_out[r] = float(x @ b)
