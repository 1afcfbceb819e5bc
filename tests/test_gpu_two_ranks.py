"""T5' (GPU): the sharded code path with the REAL kernels - two ranks sharing cuda:0, collectives over
gloo (RCCL refuses two ranks on one device; the 8-GPU node is the driver's).  Every rank must end with the
same factors, and those must match the one-rank HIP fit and the reference fixture."""
import numpy as np
import pytest

from tests.dist_common import sharded_fit, single_fit

pytestmark = pytest.mark.gpu


def _run(name, gs_mode=None, world=2):
    return sharded_fit(name, gs_mode, world, gpu=True)


def _single(name):
    return single_fit(name, gpu=True)


@pytest.mark.parametrize("name", ["g2_bias_pop", "g4_feat_uw2", "g5_graph_a0.5"])
def test_two_ranks_on_one_gpu_match_one_rank(name):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no ROCm device is visible")
    g, ref = _single(name)
    outs = _run(name)
    for key in ("U", "V", "b_u", "b_i", "rmse"):
        np.testing.assert_array_equal(outs[0][key], outs[1][key], err_msg=f"ranks disagree on {key}")
    if name == "g2_bias_pop":           # no sweep, no W-step: sharding leaves every row's arithmetic alone
        np.testing.assert_array_equal(outs[0]["U"], ref.U)
        np.testing.assert_array_equal(outs[0]["V"], ref.V)
    scale = max(np.abs(ref.V).max(), np.abs(ref.U).max())
    np.testing.assert_allclose(outs[0]["U"], ref.U, rtol=0, atol=2e-5 * scale)
    np.testing.assert_allclose(outs[0]["V"], ref.V, rtol=0, atol=2e-5 * scale)
    np.testing.assert_allclose(outs[0]["rmse"], ref.history["train_rmse"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(outs[0]["rmse"], g.d["hist_train_rmse"], rtol=0, atol=2e-5)   # and the reference
    for f in g.cfg["feats"]:
        np.testing.assert_allclose(outs[0]["W_" + f], ref.W[f], rtol=0, atol=2e-5 * max(np.abs(ref.W[f]).max(), 1e-3))


def test_block_mode_is_an_approximation_that_both_ranks_agree_on():
    outs = _run("g5_graph_a0.5", gs_mode="block")
    g, ref = _single("g5_graph_a0.5")
    np.testing.assert_array_equal(outs[0]["V"], outs[1]["V"])
    d = np.max(np.abs(outs[0]["rmse"] - np.asarray(ref.history["train_rmse"])))
    assert 0 < d < 5e-3
