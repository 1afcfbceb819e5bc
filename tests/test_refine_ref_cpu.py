"""CPU checks of solve_dtype="refine": the numpy restatement of the refinement (tests/refine_ref.py) on the fixture rows
of tests/row_auto_ref.py - what the arithmetic promises and tests/test_gpu_row_refine.py asks of the kernel - the
stopping rule on hand-made sequences, and the additive C ABI (als_row_solve_refine, als_refine_params) with the Python
switch.  No kernel is launched here."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import refine_ref as RR
from tests import row_auto_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EASY_EST = 2000.0              # rows up to this estimate must be accepted ...
EASY_STEPS = 3                 # ... within this many steps ...
EASY_ERR = 7e-9                # ... at this distance (max norm, relative to |x|) from the fp64 reference


@pytest.fixture(scope="module", params=R.KS, ids=[f"k{k}" for k in R.KS])
def batch_result(request):
    b = R.make_batch(request.param)
    return b, b.reference("f32"), RR.refine_batch(b, "f32"), RR.refine_batch(b, "f16x2")


def test_easy_rows_are_accepted_within_three_steps(batch_result):
    """Every non-empty row of at most 4096 ratings whose reference estimate is at most 2000 is accepted after at most
    3 steps and lands within 7e-9 |x| of Batch.reference(), with either Gram; its bias and statistics follow."""
    b, ref, *results = batch_result
    seen = 0
    for res in results:
        for r, rf in enumerate(ref):
            if rf is None:
                assert res[r] is None
                continue
            if rf["est"] > EASY_EST or b.lens()[r] > RR.SPLIT_CHUNK:
                continue
            seen += 1
            got = res[r]
            assert got["accepted"] and got["steps"] <= EASY_STEPS, (r, b.classes[r], got["steps"], got["why"])
            err = np.max(np.abs(got["x"] - rf["x"])) / np.max(np.abs(rf["x"]))
            print(f"k={b.k} row {r} {b.classes[r]}: est {rf['est']:.4g} steps {got['steps']} rel err {err:.2e}")
            assert err <= EASY_ERR, (r, b.classes[r], err)
            assert abs(got["bias"] - rf["bias"]) <= 1e-8 * max(1.0, abs(rf["bias"]))
            assert abs(got["sd"] - rf["sd"]) <= 1e-8 * max(1.0, rf["rho_abs"])
            assert abs(got["sd2"] - rf["sd2"]) <= 1e-8 * max(1e-3, rf["sd2"]) + 1e-12 * rf["rho2"]
    assert seen >= 20


def test_breakdown_and_split_rows_fall_back(batch_result):
    b, ref, *results = batch_result
    for res in results:
        nsplit = 0
        for r in range(b.nrows):
            if b.lens()[r] > RR.SPLIT_CHUNK:
                nsplit += 1
                assert not res[r]["accepted"] and res[r]["why"] == "split", (r, b.classes[r])
            if b.classes[r] == "breakdown" and b.k >= 50:
                assert not res[r]["accepted"], (r, res[r])
        assert nsplit >= 3


def test_accepted_rows_are_accurate_whatever_their_estimate(batch_result):
    """The rule never accepts a row that is not there: every accepted row, easy or not, is within 1e-7 |x|."""
    b, ref, *results = batch_result
    for res in results:
        for r, rf in enumerate(ref):
            if rf is not None and res[r]["accepted"]:
                err = np.max(np.abs(res[r]["x"] - rf["x"])) / np.max(np.abs(rf["x"]))
                assert err <= 1e-7, (r, b.classes[r], rf["est"], err)


def test_overfitted_rows_converge_at_once():
    """The rows the statistics flag are well conditioned: one or two steps."""
    for k in (16, 64, 150):
        b = R.make_overfit_rows(k)
        ref = b.reference("f32")
        for r, got in enumerate(RR.refine_batch(b, "f16x2")):
            if got is None:
                continue
            assert got["accepted"] and got["steps"] <= 2
            assert np.max(np.abs(got["x"] - ref[r]["x"])) <= EASY_ERR * np.max(np.abs(ref[r]["x"]))
            assert abs(got["sd2"] - ref[r]["sd2"]) <= 1e-8 * max(1e-3, ref[r]["sd2"]) + 1e-12 * ref[r]["rho2"]


def test_stopping_rule_on_hand_made_sequences():
    # steady contraction: accepted as soon as the PREDICTED next correction is below 2^-29 |x| = 1.86e-9 |x|
    assert RR.run_rule([1e-3, 1e-5, 1e-7]) == (True, 3)
    assert RR.run_rule([1e-3, 1e-6]) == (True, 2)                  # (1e-6)^2 / 1e-3 = 1e-9
    assert RR.run_rule([1e-3, 2e-6, 4e-9]) == (True, 3)            # 4e-9 is not
    assert RR.run_rule([1e-9]) == (True, 1)                        # the first correction is already negligible
    assert RR.run_rule([0.0]) == (True, 1)
    # a sequence that does not contract: given up at the first step that shrinks by less than 4, nothing accepted
    assert RR.run_rule([1e-2, 5e-3, 2.5e-3, 1.2e-3, 6e-4]) == (False, 2)
    assert RR.run_rule([1e-2, 1e-2]) == (False, 2)
    assert RR.run_rule([1e-2, 2e-2]) == (False, 2)
    # contracts by 10 a step: goes on to max_steps and falls back there
    assert RR.run_rule([1e-1, 1e-2, 1e-3, 1e-4, 1e-5]) == (False, 5)
    assert RR.run_rule([1e-1, 1e-2, 1e-3], max_steps=3) == (False, 3)
    assert RR.run_rule([1e-3, 1e-5, 1e-7], max_steps=3) == (True, 3)
    assert RR.run_rule([1e-3, 1e-5, 1e-7], max_steps=2) == (False, 2)
    # scale with |x|; non-finite corrections are never accepted
    assert RR.run_rule([1e-3, 1e-6, 1e-10], xnorm=1e-3) == (True, 3)    # what (True, 2) was at |x| = 1
    assert RR.run_rule([float("nan")]) == (False, 1)
    assert RR.run_rule([1e-3, float("inf")]) == (False, 2)


# ------------------------------------------------------------------------------------------------ C ABI, Python switch
def test_refine_entry_point_is_exported():
    from collaborative_filtering_amd import _hip
    assert "als_row_solve_refine" in _hip.EXPORTS
    lib = _hip.load()
    assert hasattr(lib, "als_row_solve_refine")
    assert lib.als_version() == 103                                 # purely additive


def test_refine_struct_layout_matches_header(tmp_path):
    from collaborative_filtering_amd import _hip
    st = _hip.RefineParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "als_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(als_refine_params));']
    src += [f'printf("%zu\\n", offsetof(als_refine_params, {f}));' for f, _ in st._fields_]
    src.append('return 0;}')
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    vals = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert C.sizeof(st) == vals[0]
    assert [getattr(st, f).offset for f, _ in st._fields_] == vals[1:]


def test_null_arguments_are_refused_without_a_device():
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    assert lib.als_row_solve_refine(None, None, None) == -1
    p, r = _hip.RowSolveParams(), _hip.RefineParams()
    assert lib.als_row_solve_refine(C.byref(p), C.byref(r), None) == -1          # cond_limit == 0


def test_solve_dtype_refine_is_accepted_and_typos_are_not():
    from collaborative_filtering_amd import ALS, ALSConfig, CoreConfig
    from collaborative_filtering_amd.backend import HipBackend
    cfg = ALSConfig(core=CoreConfig(n_factors=8, n_iters=1, lambda_u=1.0, lambda_v=1.0))
    assert ALS(cfg, solve_dtype="refine")._solve_dtype == "refine"
    with pytest.raises(ValueError):
        ALS(cfg, solve_dtype="refined")
    assert "refine" in HipBackend.SOLVE_DTYPES and HipBackend.REFINE_MAX_STEPS == 5
    import torch
    with pytest.raises(ValueError):
        HipBackend(torch.device("cpu"), solve_dtype="refined")
