"""Device-side containers of a fit, shared by the engine (engine.py), the input checks (validate.py) and the sweep
driver (sweep.py): the ratings in HBM (`_SideDev`), the row-solve task lists (`_TasksDev`), rank-local by-product
arrays (`_RowShift`), and the set-up cache of many fits on the same resident inputs (`FitCache`)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import layout


@dataclass
class _SideDev:
    nrows: int
    ncols: int
    indptr: torch.Tensor
    indices: torch.Tensor
    vals: torch.Tensor


@dataclass
class _TasksDev:
    tasks: torch.Tensor
    long_rows: torch.Tensor
    ntasks: int
    nlong: int
    nslots: int
    nnz: int
    ndual: int = 0
    nmid: int = 0


def _side_to_dev(s, device) -> _SideDev:
    if isinstance(s, _SideDev):
        return _SideDev(s.nrows, s.ncols, s.indptr.to(device), s.indices.to(device), s.vals.to(device))
    return _SideDev(s.nrows, s.ncols, torch.from_numpy(s.indptr).to(device), torch.from_numpy(s.indices).to(device),
                    torch.from_numpy(s.vals).to(device))


class _RowShift:
    """A by-product array that exists for the rank's own rows [row0, row0 + rows) only, addressed by the kernels
    with ABSOLUTE row ids: data_ptr() is moved back by row0 rows (never dereferenced outside the local rows; the
    C ABI takes plain pointers).  Everything else is the underlying tensor's."""

    def __init__(self, t: torch.Tensor, row0: int, row_elems: int):
        self.t, self.row0, self.row_elems = t, int(row0), int(row_elems)
        self.base = t                   # the tensor that exists (an attribute no torch.Tensor has)

    def data_ptr(self) -> int:
        return self.t.data_ptr() - self.row0 * self.row_elems * self.t.element_size()

    def __getattr__(self, name):
        return getattr(self.t, name)


def _to_dev(a, device, dtype) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def _tasks_to_dev(t: layout.RowTasks, device) -> _TasksDev:
    return _TasksDev(torch.from_numpy(t.tasks).to(device), torch.from_numpy(t.long_rows).to(device),
                     int(t.tasks.shape[0]), int(t.long_rows.shape[0]), t.nslots, t.nnz, t.ndual, t.nmid)


class FitCache:
    """Set-up products shared by many fits on the SAME resident inputs (sweep.SweepDriver: the tuner's
    150 x 3 fits, scripts/tune_params.py:341-421): ratings already in HBM, host copies of the row pointers, task
    lists, the similarity graph and its level schedule, uploaded features, and the (seed, shape, k)-determined
    initial factors.  Keys carry everything a value depends on; objects keyed by identity are pinned so that
    their id cannot be recycled."""

    def __init__(self):
        self._d = {}
        self._pins = []
        self.hits = 0
        self.misses = 0

    def pin(self, obj):
        self._pins.append(obj)
        return id(obj)

    def has(self, key) -> bool:
        return key in self._d

    def get(self, key, build):
        if key in self._d:
            self.hits += 1
            return self._d[key]
        self.misses += 1
        v = self._d[key] = build()
        return v
