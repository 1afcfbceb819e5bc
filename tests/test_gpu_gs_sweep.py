"""Kernel-level tests (GPU) of the Gauss-Seidel Laplacian sweep, every form against the isolated fp64 reference of
tests/gs_sweep_ref.py: als_gs_sweep (one level per call), als_gs_sweep_levels (fp32 and fp64 by-products) and
als_gs_sweep_dataflow (with and without the non-dependency pre-pass, image and stream form), with the fused residual
statistics wherever the entry point has them.  The fixture (hubs of 129+ neighbours, rows of exactly 64 and 65, 100+
wait edges in one row, a chain of 45 levels, inactive neighbours, levels of 1 / odd / non-multiple-of-4 size) and the
reference are validated without a device by tests/test_gs_sweep_ref_cpu.py, which also shows that one stale or one
too-fresh row fails `check`.

Schedules and wait lists are the production helpers' (layout.build_level_schedule, layout.wait_edges), and the dataflow
kernel is only ever given the whole schedule in its own order: no test goes near the dependency time-out."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import gs_sweep_ref as ref
from tests.gpu_common import GsSweep, env, same_bits

pytestmark = pytest.mark.gpu

STREAM_KS = (72, 96, 112, 128, 144, 150, 160)       # the stream form exists for k > 64


def _same(a, b):
    return all((x is None and y is None) or same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("k", ref.K_LIST)
def test_level_sweep_fp32(k):
    """als_gs_sweep_levels over the whole schedule (k_gs_level); fused statistics where the fp32 form has them."""
    case = ref.make_case(k)
    stat = case.ld <= 64
    V, bias, st = GsSweep(env(), case, stat=stat).levels()
    ref.check(case, V, bias, st, ref.TOL_FP32, key=f"gs level fp32 k={k}")


@pytest.mark.parametrize("k", [40, 96, 160])
def test_levels_call_is_bitwise_the_per_level_calls(k):
    """als_gs_sweep_levels == one als_gs_sweep call per level (WPW 4, 2 and 1)."""
    case = ref.make_case(k)
    E = env()
    stat = case.ld <= 64
    a = GsSweep(E, case, stat=stat).levels()
    b = GsSweep(E, case, stat=stat).level_by_level()
    assert _same(a, b)
    ref.check(case, b[0], b[1], b[2], ref.TOL_FP32)


@pytest.mark.parametrize("k", ref.K_LIST)
def test_level_sweep_f64(k):
    """k_gs_level_f64 on fp64 by-products of the fp64 row solve: the error is the fp32 rounding of the stored outputs."""
    case = ref.make_case(k)
    V, bias, st = GsSweep(env(), case, f64=True).levels()
    ref.check(case, V, bias, st, ref.TOL_F64, key=f"gs level f64 k={k}")


@pytest.mark.parametrize("k", ref.K_LIST)
def test_dataflow_sweep(k):
    """als_gs_sweep_dataflow in the form the library picks (k <= 64: registers, k > 64: image): against the reference;
    with the non-dependency pre-pass and run again: bitwise the same; and again on the SAME, not reset publication
    buffer from V_old' = -V_old, where a row left over from the previous sweep would be a wrong dependency."""
    case = ref.make_case(k)
    E = env()
    publish = E.torch.empty(case.n, case.ld, dtype=E.torch.float32, device=E.dev)
    first = GsSweep(E, case).dataflow(publish)
    ref.check(case, *first, ref.TOL_FP32, key=f"gs dataflow k={k}")
    nondep = E.torch.full((case.n, case.ld), float("nan"), dtype=E.torch.float32, device=E.dev)
    assert _same(first, GsSweep(E, case).dataflow(E.torch.empty_like(publish), nondep=nondep))
    assert _same(first, GsSweep(E, case).dataflow(E.torch.empty_like(publish)))
    flipped = case.with_v_old(-case.V_old)
    ref.check(flipped, *GsSweep(E, flipped).dataflow(publish), ref.TOL_FP32)


_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import gs_sweep_ref as ref
from tests.gpu_common import GsSweep, env
E = env()
out = {}
for k in %r:
    case = ref.make_case(k)
    publish = E.torch.empty(case.n, case.ld, dtype=E.torch.float32, device=E.dev)
    V, bias, st = GsSweep(E, case).dataflow(publish)
    out.update({f"V{k}": V, f"b{k}": bias, f"s{k}": st})
np.savez(sys.argv[1], **out)
'''


def test_dataflow_stream_form(tmp_path):
    """The stream form of k_gs_dataflow (k > 64; the library picks it above 256 items per resident wave): forced by
    ALS_GS_FORM, which is read once per process - hence ONE fresh child process for all cases."""
    env()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "stream.npz")
    res = subprocess.run([sys.executable, "-c", _CHILD % (root, STREAM_KS), out], env=dict(os.environ, ALS_GS_FORM="stream"),
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.load(out)
    for k in STREAM_KS:
        ref.check(ref.make_case(k), got[f"V{k}"], got[f"b{k}"], got[f"s{k}"], ref.TOL_FP32, key=f"gs dataflow stream k={k}")


def test_sweep_rejects_what_it_cannot_do():
    """Argument validation only: every call returns before anything is launched."""
    E = env()
    bad = r"failed with status -1\b"
    case = ref.make_case(96)
    publish = E.torch.empty(case.n, case.ld, dtype=E.torch.float32, device=E.dev)
    err = E.torch.zeros(1, dtype=E.torch.int32, device=E.dev)
    g = GsSweep(E, case, f64=True)
    with pytest.raises(RuntimeError, match=bad):                      # fp64 by-products: level launches only
        g.be.gs_dataflow(items=g.items, S_idx_wait=g.wait, publish=publish, err=err, **g.kw)
    g = GsSweep(E, case)
    with pytest.raises(RuntimeError, match=bad):                      # fused statistics of the fp32 level form: ld <= 64
        g.be.gs_levels(offsets=g.offsets, items=g.items, **g.kw)
    with pytest.raises(RuntimeError, match=bad):
        g.be.gs_level(items=g.items[:1], **g.kw)
    for missing in ("sumr2", "lambda_eff"):                           # statistics need both
        kw = dict(g.kw, **{missing: None})
        with pytest.raises(RuntimeError, match=bad):
            g.be.gs_dataflow(items=g.items, S_idx_wait=g.wait, publish=publish, err=err, **kw)
    g16 = GsSweep(E, ref.make_case(16))
    for missing in ("sumr2", "lambda_eff"):
        with pytest.raises(RuntimeError, match=bad):
            g16.be.gs_level(items=g16.items[:1], **dict(g16.kw, **{missing: None}))
    for ld in (case.ld - 16, case.ld + 16, case.ld + 1):                 # ld is padded_k(k), nothing else
        with pytest.raises(RuntimeError, match=bad):
            g.be.gs_level(items=g.items[:1], **dict(g.kw, ld=ld, stat_out=None))
        with pytest.raises(RuntimeError, match=bad):
            g.be.gs_dataflow(items=g.items, S_idx_wait=g.wait, publish=publish, err=err, **dict(g.kw, ld=ld))
    E.torch.cuda.synchronize()
    for g_ in (g, g16):                                               # nothing ran
        assert same_bits(g_.V.cpu(), g_.case.V_pad()) and same_bits(g_.bias.cpu(), g_.case.b_i)
    assert int(err.item()) == 0
