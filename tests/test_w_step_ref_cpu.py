"""The W-step reference of tests/w_step_ref.py, validated without a device: against the reference algorithm's explicit
design matrix, against the engine's numpy stand-in (tests/cpu_backend.py), and against the direct residual sums; plus
the promises its case table makes to tests/test_gpu_w_step.py (exact magnitudes, edge coverage)."""
import numpy as np
import pytest
import torch

from tests import w_step_ref as ref
from tests.cpu_backend import NumpyBackend

TINY = dict(n=12, ib=2, ie=11, nchunks=2, dims=[1, 3], kinds=["dense", "even", "last"])


def _tiny(k, feat, kind="real", f64=True):
    kinds = TINY["kinds"][: TINY["dims"][feat]]
    return ref.build_inputs(k=k, kind=kind, f64=f64, seed=10 * k + feat, feat=feat,
                            **{**TINY, "kinds": kinds})


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)))
                 / max(np.max(np.abs(np.asarray(b, dtype=np.float64))), 1e-300))


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("feat", [0, 1])                       # d = 1 and d = 3
@pytest.mark.parametrize("k", [3, 20])
def test_reference_equals_the_explicit_design_matrix(k, feat, kind):
    """Reference algorithm, W-step: every rating (u, i) gives the row x_i (x) U_u of the N_obs x (d k) design matrix;
    the target is the residual with the old W of the other features included and of this feature excluded."""
    inp = _tiny(k, feat, kind)
    d, c0 = inp.dims[feat], int(inp.feat_off[feat])
    W = inp.W.astype(np.float64)
    rows, target = [], []
    for i in range(inp.ib, inp.ie):
        x = inp.X[i].astype(np.float64)
        others = inp.V[i, :k].astype(np.float64) + x @ W - x[c0:c0 + d] @ W[c0:c0 + d]
        for u in range(int(inp.ni[i])):
            Uu = inp.users_U[i, u]
            rows.append(np.outer(x[c0:c0 + d], Uu).reshape(d * k))
            target.append(inp.users_rho[i, u] - float(inp.b_new[i]) - Uu @ others)
    M, t = np.array(rows), np.array(target)
    H, _ = ref.expected_h(inp, wide=True)
    A, _, B, _ = ref.expected_ab(inp, H[feat], wide=True)
    assert _rel(A, M.T @ M) <= 1e-12 and _rel(B, M.T @ t) <= 1e-12


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("k", [3, 20])
def test_reference_agrees_with_the_numpy_stand_in(k, f64):
    inp = _tiny(k, 1, "real", f64)
    tt = torch.from_numpy
    Wld = np.zeros((inp.D, inp.ld))
    Wld[:, :k] = inp.W[:, :k]
    be = NumpyBackend()
    Hs = torch.zeros(inp.nfeat, inp.n, inp.ld, dtype=torch.float32)
    be.w_item_vectors(k=k, ld=inp.ld, item_begin=inp.ib, item_end=inp.ie, gram=tt(inp.gram), rhs=tt(inp.rhs),
                      colsum=tt(inp.colsum), V=tt(inp.V), b_new=tt(inp.b_new), b_old=tt(inp.b_old), X=tt(inp.X),
                      feat_off=tt(inp.feat_off), W=tt(Wld), H=Hs)
    H, S = ref.expected_h(inp)
    sl = slice(inp.ib, inp.ie)
    got = Hs.numpy()[:, sl].astype(np.float64)
    # the stand-in stores float32: one rounding of H, plus fp64 evaluation noise relative to the companion
    assert np.all(np.abs(got - H[:, sl]) <= ref.U32 * np.abs(H[:, sl]) + 1e-13 * S[:, sl])
    A, SA, B, SB = ref.expected_ab(inp, Hs.numpy()[1])
    As, Bs = be.w_accumulate(k=k, ld=inp.ld, item_begin=inp.ib, item_end=inp.ie, gram=tt(inp.gram), X=tt(inp.X), H=Hs,
                             feat_index=1, feat_col0=int(inp.feat_off[1]), feat_d=inp.dims[1])
    assert _rel(As.numpy(), A) <= 1e-12 and _rel(Bs.numpy(), B) <= 1e-12


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("k", [3, 20])
def test_closed_form_statistics_equal_the_direct_sums(k, kind):
    inp = _tiny(k, 1, kind)
    stat, S = ref.expected_stats(inp, wide=True)
    for i in range(inp.ib, inp.ie):
        nu = int(inp.ni[i])
        d = inp.users_rho[i, :nu] - float(inp.b_new[i]) - inp.users_U[i, :nu] @ inp.Z[i, :k].astype(np.float64)
        assert abs(float(stat[i, 0]) - d.sum()) <= 1e-10 * float(S[i, 0]) + 1e-300
        assert abs(float(stat[i, 1]) - (d * d).sum()) <= 1e-10 * float(S[i, 1]) + 1e-300
    assert np.isnan(np.asarray(stat[: inp.ib], dtype=np.float64)).all()


@pytest.mark.parametrize("k", sorted(ref.CASES))
def test_exact_inputs_keep_their_magnitude_bounds(k):
    cfg = ref.CASES[k]
    inp = ref.build_inputs(k=k, kind="exact", f64=False, seed=k, **cfg)       # asserts them itself
    ref.check_exact_magnitudes(inp)
    # what must not be read is poisoned: upper blocks everywhere, whole rows outside the shard
    blk = np.arange(inp.ld) // 16
    assert np.isnan(inp.gram[:, blk[:, None] < blk[None, :]]).all()
    assert not np.isnan(inp.gram[inp.ib:inp.ie][:, blk[:, None] >= blk[None, :]]).any()
    for a in (inp.gram, inp.rhs, inp.colsum, inp.X, inp.b_new, inp.b_old, inp.V):
        assert np.isnan(a[: inp.ib]).all() and np.isnan(a[inp.ie:]).all()


def test_case_table_covers_every_edge():
    """Every edge the GPU test promises occurs in at least one parametrised case."""
    cases = [dict(k=k, **c) for k, c in ref.CASES.items()] + list(ref.EXTRA_CASES.values())
    assert {c["k"] for c in cases} >= {1, 8, 16, 24, 40, 50, 64, 72, 96, 100, 128, 144, 150, 160}
    assert {-(-c["k"] // 16) for c in cases} == set(range(1, 11))
    seen = set()
    for c in cases:
        for kind in ("exact", "real"):
            rng = np.random.default_rng(c["k"])
            kw = {x: c[x] for x in ("n", "ib", "ie", "nchunks", "dims", "feat", "kinds")}
            X, off = ref.build_x(rng, kind=kind, **kw)
            ib, ie, nch, d, c0 = c["ib"], c["ie"], c["nchunks"], c["dims"][c["feat"]], int(off[c["feat"]])
            tiles = ref.chunk_tiles(ib, ie, nch)
            lens = {}
            for ch, t0, t1 in tiles:
                lens[ch] = lens.get(ch, 0) + t1 - t0
            seen |= {("nchunks", nch), ("d", d), ("nfeat", len(c["dims"]))}
            seen |= {("chunk", 256) for v in lens.values() if v == 256}
            seen |= {("chunk", 257) for v in lens.values() if v == 257}
            seen |= {("chunk", ">512") for v in lens.values() if v > 512}
            if len(lens) < nch:
                seen.add("empty chunk")
            if c0 > 0 and c["feat"] >= 1:
                seen.add("feature offset")
            if 0 < ib < ie < c["n"]:
                seen.add("inner shard")
            counts = ref.tile_counts(X, ib, ie, nch, c0, d)
            for (a, a2, t0), cnt in counts.items():
                full = min(t1 for _, s, t1 in tiles if s == t0) - t0
                seen.add((kind, "mod4", cnt % 4))
                if cnt == 0:
                    seen.add((kind, "empty tile"))
                if cnt == 256 and full == 256:
                    seen.add((kind, "full tile"))
            Xs = X[ib:ie, c0:c0 + d]
            for a in range(d):
                nz = np.flatnonzero(Xs[:, a])
                if nz.size == 1 and nz[0] == ie - ib - 1:
                    seen.add((kind, "last item only"))
                for a2 in range(a + 1, d):
                    if Xs[:, a].any() and Xs[:, a2].any() and not (Xs[:, a] * Xs[:, a2]).any():
                        seen.add((kind, "disjoint pair"))
    want = {("nchunks", 1), ("nchunks", 2), ("nchunks", 3), ("chunk", 256), ("chunk", 257), ("chunk", ">512"),
            "empty chunk", "feature offset", "inner shard", ("d", 1), ("d", 3), ("d", 20),
            ("nfeat", 1), ("nfeat", 2), ("nfeat", 3), ("nfeat", 8)}
    for kind in ("exact", "real"):
        want |= {(kind, "mod4", r) for r in range(4)}
        want |= {(kind, "empty tile"), (kind, "full tile"), (kind, "last item only"), (kind, "disjoint pair")}
    assert want <= seen, want - seen
    w = ref.EXTRA_CASES["wrapper"]
    npairs = w["dims"][0] * (w["dims"][0] + 1) // 2
    nchunks = max(1, min(512, 4096 // npairs, -(-w["n"] // 64)))           # HipBackend.w_accumulate
    assert nchunks == w["nchunks"] == 19 and -(-w["n"] // nchunks) > 256
