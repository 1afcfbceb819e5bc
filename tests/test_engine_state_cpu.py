"""The engine's state is complete after construction: no method creates an attribute later, and every attribute a
method reads exists on every path (None / False where it does not apply) - with or without features, graph, fused
statistics, on the numpy stand-in and on the HIP backend, eagerly and under captured-graph replay."""
import pytest

from tests.common import Golden, model_for

FIXTURES = ["g1_plain", "g4_feat_uw5", "g5_graph_a0.5", "g10_full_k64"]
# what reads of the form getattr(eng, name, default) / hasattr(eng, name) used to ask for
ONCE_GUARDED = ("gs_dataflow", "gs_mode", "gs_nondep", "X64", "H", "b_i_prev", "utasks_c")
# (fused_stats, fused_feat_stats, use_graph) on the numpy stand-in, which has sum_pairs but no item_stats
PATHS_CPU = {"g1_plain": (True, False, False), "g4_feat_uw5": (False, False, False),
             "g5_graph_a0.5": (False, False, True), "g10_full_k64": (False, False, True)}
# the same on the HIP backend (sum_pairs, item_stats, gs_dataflow): every fixture but the first has features
PATHS_HIP = {"g1_plain": (True, False, False), "g4_feat_uw5": (False, True, False),
             "g5_graph_a0.5": (False, True, True), "g10_full_k64": (False, True, True)}


def _engine(name, **kw):
    from collaborative_filtering_amd import layout
    g = Golden(name)
    r, c, v = g.train
    csr, csc = layout.coo_to_sides(r, c, v, (g.m, g.n))
    model = model_for(g, **kw)
    eng = model.prepare_csr((csr.indptr, csr.indices, csr.vals), (csc.indptr, csc.indices, csc.vals), (g.m, g.n),
                            features=g.features or None)
    return model, eng                   # (the engine holds the model weakly)


def _check_state_is_fixed(eng, n_iters, paths):
    before = set(vars(eng))
    for it in range(n_iters):
        eng.iteration(it, n_iters)
    eng._check_status()
    after = set(vars(eng))
    assert after == before, sorted(after ^ before)
    assert not [a for a in ONCE_GUARDED if a not in after]
    assert (bool(eng.fused_stats), bool(eng.fused_feat_stats), bool(eng.use_graph)) == paths
    assert (eng.gs_mode is None) == (not eng.use_graph) and (eng.H is None) == (not eng.feat_names)


@pytest.mark.parametrize("name", FIXTURES)
def test_engine_state_is_complete_after_construction_cpu(name):
    from tests.cpu_backend import NumpyBackend
    model, eng = _engine(name, device="cpu", backend=NumpyBackend())
    _check_state_is_fixed(eng, 2, PATHS_CPU[name])
    assert eng.gs_dataflow is False and not eng.native


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_engine_state_is_complete_after_construction_hip(name):
    """The HIP backend takes the other side of every capability branch: rank-local `_RowShift` by-products, the
    dataflow sweep, `item_stats`, `history_row`."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no ROCm device is visible")
    model, eng = _engine(name)
    _check_state_is_fixed(eng, 2, PATHS_HIP[name])
    assert eng.native and eng.has_item_stats and eng.has_history_row and eng.has_gs_levels


@pytest.mark.gpu
def test_engine_state_is_fixed_under_captured_graph_replay():
    """Three iterations with hip_graph=True: the first runs eagerly, the second is captured, the third replays.
    Nothing may be created on the engine during capture."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no ROCm device is visible")
    model, eng = _engine("g10_full_k64", hip_graph=True)
    _check_state_is_fixed(eng, 3, PATHS_HIP["g10_full_k64"])
    assert eng.graphs_captured > 0
