"""T3 (GPU): the fold of a split row's partial slots (k_sum_slots / k_sum_slots_f64, csrc/slot_fold.hpp) through
als_row_solve, as tests/test_gpu_kernels.py calls it.

A row of more than ALS_SPLIT_CHUNK ratings is cut into segments whose partial normal equations go to consecutive
workspace slots; the fold sums them into the row's first slot in ascending slot order and k_row_long finishes the
row from there.  Two checks per split row:
  1. the row's solution and bias against the numpy fp64 solve of tests/cpu_backend.py, within the whole-row
     tolerances of test_gpu_kernels.test_row_solve_against_numpy;
  2. slot 0 of the workspace after the call equals BITWISE the sum  0 + w[0], += w[1], ..., += w[nslots-1]  of the
     partials (fp32 adds; the fp64 kernel: w[0], += w[1], ... in doubles).  The partials are read back by a call with
     only the row's segment tasks and nlong = 0: the main kernel writes them, the fold is what is under test.
The fold takes the slots in blocks of B = ALS_SLOT_FOLD_BLOCK with a shorter first block, two register sets and a
steady-state loop from three full blocks on, so the slot counts sit around B, 2 B, 3 B and 4 B."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests.cpu_backend import NumpyBackend
from tests.gpu_common import env, pad, random_side

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(path, name):
    text = open(os.path.join(_ROOT, path)).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


CHUNK = _define("include/als_hip.h", "ALS_SPLIT_CHUNK")
B = _define("collaborative-filtering_amd/csrc/slot_fold.hpp", "ALS_SLOT_FOLD_BLOCK")
ORDINARY = [1, 2, 9, 16, 17, 40, 64, 65, 100, 300, 700, CHUNK]      # a dozen rows that are not split
LAST_SEG = 5                                                        # ratings of a split row's last segment

# whole-row tolerances of test_gpu_kernels.test_row_solve_against_numpy: x relative to max|x| of the row, bias
# relative to max(1, |bias|)
TOL = {"f16x2": (6e-5, 2e-6), "f64": (6e-7, 6e-7)}


def _solve(k, gram, nslots_list, seed):
    """One als_row_solve over rows split into `nslots_list` slots plus the ordinary rows.  Returns what the checks
    need: outputs, the workspace after the full call and after the partials-only call, the reference solution."""
    torch, layout, side_dev, tasks_dev, be, dev = env(gram)
    from collaborative_filtering_amd.als import _TasksDev
    assert layout.SPLIT_CHUNK == CHUNK
    lens = [(n - 1) * CHUNK + LAST_SEG for n in nslots_list] + ORDINARY
    nrows, ncols = len(lens), max(lens) + 1000
    side = random_side(layout, nrows, ncols, lens, seed=seed)
    rng = np.random.default_rng(seed + 1)
    ld = layout.padded_k(k)
    F = pad(rng.normal(scale=0.3, size=(ncols, k)), ld, 1)
    b_self = rng.normal(scale=0.2, size=nrows).astype(np.float32)
    b_other = rng.normal(scale=0.2, size=ncols).astype(np.float32)
    mu, lam, lam_b = 3.3, 2.5, 1.7
    t = layout.build_row_tasks(side.indptr)
    assert [int(n) for n in t.long_rows[:, 2]] == list(nslots_list) and t.nslots == sum(nslots_list)
    sd = side_dev(side, dev)
    f32 = torch.float32
    nwords = be.slot_bytes(k) // 4
    wdtype = np.float64 if gram == "f64" else np.float32

    def call(td):
        X_out = torch.full((nrows, ld), 7.0, dtype=f32, device=dev)
        bias_out = torch.full((nrows,), 7.0, dtype=f32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.zeros(t.nslots * nwords, dtype=f32, device=dev)
        be.row_solve(k=k, ld=ld, side=sd, F=torch.from_numpy(F).to(dev), zero_row=ncols,
                     bias_self=torch.from_numpy(b_self).to(dev), bias_other=torch.from_numpy(b_other).to(dev),
                     mu=torch.tensor([mu], dtype=torch.float64, device=dev), lam=lam, lam_row=None, lam_b=lam_b,
                     lam_b_row=None, rhs_extra=None, diag_extra=None, X_out=X_out, bias_out=bias_out, gram_out=None,
                     factor_out=None, rhs_out=None, colsum_out=None, sumr_out=None, status=status, tasks=td,
                     workspace=ws)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        w = ws.cpu().numpy().view(wdtype).reshape(t.nslots, -1)
        return X_out.cpu().numpy(), bias_out.cpu().numpy(), w

    X, bias, ws_full = call(tasks_dev(t, dev))
    seg = np.ascontiguousarray(t.tasks[t.tasks[:, 2] >= 0])                 # the segment tasks of the split rows
    assert seg.shape[0] == t.nslots
    only_segments = _TasksDev(torch.from_numpy(seg).to(dev), torch.zeros((0, 4), dtype=torch.int32, device=dev),
                              int(seg.shape[0]), 0, t.nslots, t.nnz, 0, 0)
    _, _, ws_part = call(only_segments)

    # reference: numpy fp64 on the same fp32 inputs
    cpu = SimpleNamespace(indptr=torch.from_numpy(side.indptr), indices=torch.from_numpy(side.indices),
                          vals=torch.from_numpy(side.vals), nrows=nrows)
    X_ref = torch.zeros(nrows, ld, dtype=f32)
    bias_ref = torch.zeros(nrows, dtype=f32)
    NumpyBackend(np.float64).row_solve(
        k=k, ld=ld, side=cpu, F=torch.from_numpy(F), zero_row=ncols, bias_self=torch.from_numpy(b_self),
        bias_other=torch.from_numpy(b_other), mu=torch.tensor([mu], dtype=torch.float64), lam=lam, lam_row=None, lam_b=lam_b, lam_b_row=None,
        rhs_extra=None, diag_extra=None, X_out=X_ref, bias_out=bias_ref, gram_out=None, factor_out=None,
        rhs_out=None, colsum_out=None, sumr_out=None, status=torch.zeros(1, dtype=torch.int32),
        tasks=SimpleNamespace(tasks=torch.from_numpy(t.tasks)), workspace=None)
    return SimpleNamespace(k=k, gram=gram, long_rows=t.long_rows, X=X, bias=bias, ws_full=ws_full, ws_part=ws_part,
                           X_ref=X_ref.numpy(), bias_ref=bias_ref.numpy(), nrows=nrows)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _check(r):
    xa, ba = TOL[r.gram]
    # pass 1: every row (the split ones among them) against the fp64 solve
    for row in range(r.nrows):
        x = r.X_ref[row, :r.k].astype(np.float64)
        scale = max(np.max(np.abs(x)), 1e-6)
        np.testing.assert_allclose(r.X[row, :r.k], x, rtol=0, atol=xa * scale, err_msg=f"row {row}")
        assert np.all(r.X[row, r.k:] == 0.0)
        bref = float(r.bias_ref[row])
        assert abs(float(r.bias[row]) - bref) <= ba * max(1.0, abs(bref)), (row, r.bias[row], bref)
    # pass 2: slot 0 is the ascending-order sum of the partials, bit for bit; the other slots are left alone
    for row, slot0, nslots, _ in r.long_rows:
        w = r.ws_part[slot0:slot0 + nslots]
        if r.gram == "f64":
            acc = w[0].copy()
        else:
            acc = np.zeros_like(w[0]) + w[0]
        assert acc.dtype == w.dtype
        for s in range(1, nslots):
            acc = acc + w[s]                                    # one IEEE add per element, in slot order
        assert np.any(w[nslots - 1] != 0) and np.any(acc != w[0])
        np.testing.assert_array_equal(_bits(r.ws_full[slot0]), _bits(acc), err_msg=f"row {row} nslots {nslots}")
        np.testing.assert_array_equal(_bits(r.ws_full[slot0 + 1:slot0 + nslots]), _bits(w[1:]))


# around the block size (the first block is the short one: nslots - 1 = q B + rem), and from three full blocks on,
# where the two register sets alternate in a loop: 3 B + 1 leaves it with one block, 4 B + 6 with two
SLOT_COUNTS = [2, 3, B, B + 1, B + 2, 2 * B, 2 * B + 1, 2 * B + 3]
LOOP_SLOT_COUNTS = [3 * B + 1, 4 * B + 6]


@pytest.mark.parametrize("nslots", SLOT_COUNTS + LOOP_SLOT_COUNTS)
def test_fold_one_split_row(nslots):
    _check(_solve(16, "f16x2", [nslots], seed=1000 + nslots))


def test_fold_rows_of_very_different_slot_counts():
    _check(_solve(16, "f16x2", [2, 7, 2 * B + 3, 3, 3 * B + 2], seed=2000))


@pytest.mark.parametrize("k", [64, 128])
def test_fold_wide_slots(k):
    """more than one vector group per slot; k = 128 is the KB = 8 layout"""
    _check(_solve(k, "f16x2", [B + 1], seed=3000 + k))


@pytest.mark.parametrize("nslots", SLOT_COUNTS)
@pytest.mark.parametrize("k", [16, 64])
def test_fold_f64(k, nslots):
    _check(_solve(k, "f64", [nslots], seed=4000 + 100 * k + nslots))


def test_fold_f64_loop():
    _check(_solve(16, "f64", [3 * B + 1, 4 * B + 6], seed=5000))


def test_fold_is_deterministic():
    a = _solve(16, "f16x2", [2 * B + 3], seed=6000)
    b = _solve(16, "f16x2", [2 * B + 3], seed=6000)
    np.testing.assert_array_equal(_bits(a.X), _bits(b.X))
    np.testing.assert_array_equal(_bits(a.bias), _bits(b.bias))
    np.testing.assert_array_equal(_bits(a.ws_full), _bits(b.ws_full))
