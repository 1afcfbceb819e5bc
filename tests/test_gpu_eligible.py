"""K8 / K11 segmented and K20 (GPU): als_recommend_topk_segmented, als_rank_count_segmented (the SEG instantiations of
k_recommend and k_rank_count), als_eligibility_bitmaps (csrc/eligibility.hip) and the ALS.*_eligible calls.

The oracle of the two segmented kernels is their definition: row b equals, element for element, row b of
als_recommend_topk_masked / als_rank_count_masked called with allow = E[row_seg[b]] - here one masked call per segment
over the rows of that segment (a row's result does not depend on the other rows of its batch).  The builder is held
to the numpy definition of tests/eligible_ref.py.  Every comparison is ==, and every output buffer starts from a poison
value: a slot the call does not write fails the comparison."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import eligible_ref as eref
from tests.common import Golden, model_for
from tests.gpu_common import assert_same, env, factors, ptr as cptr, run_rank, run_topk, seen_csr, upload
from tests.serving_ref import bitmap_numpy

POISON_WORD = 0x77777777


def five_segments(n, seed, pad_words=0):
    """The table of the kernel tests, uint32 [5, W + pad_words]: all ones; all zero; one single item; random 50 %; only
    the last (partial) word - with the bits >= n set as well, which every reader has to ignore.  Padding words (a row
    stride above W) hold garbage."""
    rng = np.random.default_rng(seed)
    W = (n + 31) // 32
    E = np.zeros((5, W + pad_words), dtype=np.uint32)
    E[0, :W] = bitmap_numpy(np.ones(n, bool))
    one = np.zeros(n, bool)
    one[int(rng.integers(0, n))] = True
    E[2, :W] = bitmap_numpy(one)
    E[3, :W] = bitmap_numpy(rng.random(n) < 0.5)
    E[4, W - 1] = 0xFFFFFFFF
    E[:, W:] = 0xA5A5A5A5
    return E


def run_topk_seg(torch, be, f, users, n, seen_ptr, seen_idx, N, dev, table_d, row_seg):
    """als_recommend_topk_segmented into poisoned buffers -> numpy (values, items, counts)."""
    us = upload(np.asarray(users, np.int32), dev)
    B = us.numel()
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), -7, dtype=torch.int32, device=dev)
    be.recommend_topk_segmented(k=f["k"], ld=f["ld"], users=us, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"],
                                mu=f["mu"], seen_ptr=None if seen_ptr is None else upload(seen_ptr, dev),
                                seen_idx=None if seen_idx is None else upload(seen_idx, dev), seg_allow=table_d,
                                row_seg=upload(np.asarray(row_seg, np.int32), dev), topn=N, top_val=tv, top_idx=ti,
                                top_cnt=tc)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()


def masked_per_segment(torch, be, f, users, n, seen_ptr, seen_idx, N, dev, E, row_seg):
    """The oracle: als_recommend_topk_masked with allow = E[s] over the rows of every segment s."""
    W = (n + 31) // 32
    users, row_seg = np.asarray(users), np.asarray(row_seg)
    tv = np.full((users.size, N), 7.0, np.float32)
    ti = np.full((users.size, N), -7, np.int32)
    tc = np.full(users.size, -7, np.int32)
    for s in np.unique(row_seg):
        rows = np.nonzero(row_seg == s)[0]
        allow = upload(np.ascontiguousarray(E[s, :W]).view(np.int32), dev)
        tv[rows], ti[rows], tc[rows] = run_topk(torch, be, f, users[rows], n, seen_ptr, seen_idx, N, dev, allow=allow)
    return tv, ti, tc


def table_dev(E, dev):
    return upload(np.ascontiguousarray(E).view(np.int32), dev)


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("k", [1, 50, 64, 128, 160])
@pytest.mark.parametrize("n", [1, 33, 200, 4099])
def test_kernel_equals_per_segment_masked_call(k, n):
    torch, layout, be, dev = env().short
    m = 60
    f = factors(torch, layout, dev, m, n, k, seed=10 * k + n)
    ptr, idx, rows = seen_csr(m, n, seed=k + n)
    rng = np.random.default_rng(k * n)
    # 150 batch rows: reversed order, duplicates; 64- and 128-row workgroups both end in a partial wave
    users = np.concatenate([np.arange(m), rng.integers(0, m, 90)])[::-1].copy()
    row_seg = rng.integers(0, 5, users.size)                               # every wave mixes the segments
    E = five_segments(n, seed=n + k, pad_words=k % 3)                      # row strides W + 1 and W + 2
    Ed = table_dev(E, dev)
    for N in (10, 128):                                                    # 8-wave and 4-wave workgroups
        for sp, si in ((ptr, idx), (None, None)):
            got = run_topk_seg(torch, be, f, users, n, sp, si, N, dev, Ed, row_seg)
            assert_same(got, masked_per_segment(torch, be, f, users, n, sp, si, N, dev, E, row_seg))
            assert (got[2][row_seg == 1] == 0).all() and (got[1][row_seg == 1] == -1).all()
            assert (got[2][row_seg == 2] <= 1).all()


def test_result_does_not_depend_on_the_slice_count(monkeypatch):
    torch, layout, be, dev = env().short
    m, n, k = 150, 5003, 64
    f = factors(torch, layout, dev, m, n, k, seed=3)
    ptr, idx, rows = seen_csr(m, n, seed=4)
    rng = np.random.default_rng(5)
    users = rng.permutation(m)
    row_seg = rng.integers(0, 5, m)
    E = five_segments(n, seed=6)
    Ed = table_dev(E, dev)
    for N in (10, 128):
        outs = []
        for s in (1, 2, 7, 64):
            monkeypatch.setenv("ALS_RECOMMEND_SLICES", str(s))
            outs.append(run_topk_seg(torch, be, f, users, n, ptr, idx, N, dev, Ed, row_seg))
        monkeypatch.delenv("ALS_RECOMMEND_SLICES")
        outs.append(run_topk_seg(torch, be, f, users, n, ptr, idx, N, dev, Ed, row_seg))      # automatic
        for o in outs[1:]:
            assert_same(o, outs[0])
        assert_same(outs[0], masked_per_segment(torch, be, f, users, n, ptr, idx, N, dev, E, row_seg))


def _chunk_only(n, chunks):
    mask = np.zeros(n, bool)
    for ch in chunks:
        mask[32 * ch: 32 * ch + 32] = True
    return bitmap_numpy(mask)


@pytest.mark.parametrize("slices", ["1", None])
def test_waves_that_skip_chunks_keep_the_barriers_matched(slices, monkeypatch):
    """Waves 0 and 1 of a workgroup skip every chunk but one (a different one each) while the others score them all,
    then every wave is sparse: staging and both barriers are still taken by all, or the lists would be wrong (or the
    call would not return)."""
    torch, layout, be, dev = env().short
    if slices:
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)                 # one workgroup walks chunk 3 and chunk 100
    m, n, k = 128, 4099, 64
    f = factors(torch, layout, dev, m, n, k, seed=7)
    ptr, idx, rows = seen_csr(m, n, seed=8)
    E = np.stack([_chunk_only(n, [100]), _chunk_only(n, [3]), bitmap_numpy(np.ones(n, bool))])
    Ed = table_dev(E, dev)
    users = np.arange(m)
    mixed = np.full(m, 2)
    mixed[:16], mixed[16:32] = 0, 1
    sparse = (np.arange(m) // 16) % 2                                      # whole waves on chunk 100 or on chunk 3
    for row_seg in (mixed, sparse):
        for N in (10, 128):
            for sp, si in ((ptr, idx), (None, None)):
                got = run_topk_seg(torch, be, f, users, n, sp, si, N, dev, Ed, row_seg)
                assert_same(got, masked_per_segment(torch, be, f, users, n, sp, si, N, dev, E, row_seg))
        got = run_topk_seg(torch, be, f, users, n, None, None, 128, dev, Ed, row_seg)
        assert (got[2][row_seg == 0] == 32).all() and (got[2][row_seg == 1] == 32).all()
        assert ((got[1][row_seg == 0][:, :32] // 32) == 100).all() and ((got[1][row_seg == 1][:, :32] // 32) == 3).all()


@pytest.mark.parametrize("slices", ["1", None])
def test_seen_cursors_catch_up_after_skipped_chunks(slices, monkeypatch):
    """Seen rows that are dense inside the skipped chunks and run on into the first allowed one: the exclusion walk has
    to consume far more than 16 entries when it is first asked about a block."""
    torch, layout, be, dev = env().short
    if slices:
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n, k = 64, 1500, 50
    f = factors(torch, layout, dev, m, n, k, seed=9)
    rng = np.random.default_rng(10)
    seen = []
    for u in range(m):
        kind = u % 4
        if kind == 0:
            s = np.arange(0, 170)                                          # chunks 0 .. 4 and the first 10 of chunk 5
        elif kind == 1:
            s = np.arange(0, 192)                                          # ... and all of chunk 5: nothing left there
        elif kind == 2:
            s = np.concatenate([np.arange(150, 200), np.arange(1260, 1290)])       # across both ends of chunk 5; chunk 40
        else:
            s = np.nonzero(rng.random(n) < 0.6)[0]                         # about 19 of 32 everywhere
        seen.append(s)
    ptr = np.zeros(m + 1, np.int64)
    ptr[1:] = np.cumsum([s.size for s in seen])
    idx = np.concatenate(seen).astype(np.int32)
    E = np.stack([_chunk_only(n, [5]), _chunk_only(n, [5, 40]), _chunk_only(n, [46]), bitmap_numpy(np.ones(n, bool))])
    Ed = table_dev(E, dev)
    users = np.arange(m)
    for row_seg in (rng.integers(0, 3, m), rng.integers(0, 4, m), np.zeros(m, np.int64)):
        for N in (10, 128):
            got = run_topk_seg(torch, be, f, users, n, ptr, idx, N, dev, Ed, row_seg)
            assert_same(got, masked_per_segment(torch, be, f, users, n, ptr, idx, N, dev, E, row_seg))
    got = run_topk_seg(torch, be, f, users, n, ptr, idx, 128, dev, Ed, np.zeros(m, np.int64))
    assert (got[2][0::4] == 22).all() and (got[2][1::4] == 0).all() and (got[2][2::4] == 0).all()


def run_rank_seg(torch, be, f, users, n, seen_ptr, seen_idx, q_ptr, q_items, dev, table_d, row_seg):
    """als_rank_count_segmented into poisoned buffers -> numpy (t_score, above, n_cand)."""
    t = lambda a, dt: upload(np.asarray(a, dt), dev)        # noqa: E731
    nq, nt = len(users), len(q_items)
    sc = torch.full((nt,), 7.0, dtype=torch.float32, device=dev)
    ab = torch.full((nt,), -7, dtype=torch.int32, device=dev)
    nc = torch.full((nq,), -7, dtype=torch.int32, device=dev)
    be.rank_count_segmented(k=f["k"], ld=f["ld"], n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"],
                            seen_ptr=None if seen_ptr is None else t(seen_ptr, np.int64),
                            seen_idx=None if seen_idx is None else t(seen_idx, np.int32), seg_allow=table_d,
                            row_seg=t(row_seg, np.int32), q_users=t(users, np.int32), q_ptr=t(q_ptr, np.int64),
                            q_items=t(q_items, np.int32), t_score=sc, above=ab, n_cand=nc)
    return sc.cpu().numpy(), ab.cpu().numpy(), nc.cpu().numpy()


@pytest.mark.parametrize("k,n", [(50, 4099), (160, 200), (64, 33)])
def test_rank_count_segmented_equals_per_segment_masked_call(k, n, monkeypatch):
    torch, layout, be, dev = env().short
    m = 60
    f = factors(torch, layout, dev, m, n, k, seed=k + n)
    ptr, idx, rows = seen_csr(m, n, seed=k)
    rng = np.random.default_rng(n)
    users = np.concatenate([np.arange(m), rng.integers(0, m, 90)])[::-1].copy()
    B = users.size
    row_seg = rng.integers(0, 5, B)
    cnt = rng.integers(0, 4, B)
    cnt[7] = 40                                                            # more than 16 targets: further passes
    q_ptr = np.zeros(B + 1, np.int64)
    q_ptr[1:] = np.cumsum(cnt)
    q_items = rng.integers(0, n, q_ptr[-1])
    E = five_segments(n, seed=k, pad_words=1)
    Ed = table_dev(E, dev)
    W = (n + 31) // 32
    for s_env in ("1", "7", None):
        if s_env:
            monkeypatch.setenv("ALS_RECOMMEND_SLICES", s_env)
        else:
            monkeypatch.delenv("ALS_RECOMMEND_SLICES")
        for sp, si in ((ptr, idx), (None, None)):
            got = run_rank_seg(torch, be, f, users, n, sp, si, q_ptr, q_items, dev, Ed, row_seg)
            sc = np.full(q_items.size, 7.0, np.float32)
            ab = np.full(q_items.size, -7, np.int32)
            nc = np.full(B, -7, np.int32)
            for s in np.unique(row_seg):
                r = np.nonzero(row_seg == s)[0]
                sel = np.concatenate([np.arange(q_ptr[b], q_ptr[b + 1]) for b in r]).astype(np.int64)
                sub_ptr = np.zeros(r.size + 1, np.int64)
                sub_ptr[1:] = np.cumsum(cnt[r])
                allow = upload(np.ascontiguousarray(E[s, :W]).view(np.int32), dev)
                o = run_rank(torch, be, f, users[r], n, sp, si, sub_ptr, q_items[sel], dev, allow=allow)
                sc[sel], ab[sel], nc[r] = o
            assert_same(got, (sc, ab, nc))
    # an item the segmented top-N returns at position j has above == j
    N = 128
    tv, ti, tc = run_topk_seg(torch, be, f, users, n, ptr, idx, N, dev, Ed, row_seg)
    bb, jj = np.nonzero(ti >= 0)
    t_ptr = np.zeros(B + 1, np.int64)
    t_ptr[1:] = np.cumsum(tc)
    sc, ab, nc = run_rank_seg(torch, be, f, users, n, ptr, idx, t_ptr, ti[bb, jj], dev, Ed, row_seg)
    assert (ab == jj).all() and (sc == tv[bb, jj]).all() and (nc >= tc).all()


@pytest.mark.parametrize("tw", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4099])
def test_eligibility_bitmaps_against_numpy(tw, n):
    torch, layout, be, dev = env().short
    rng = np.random.default_rng(100 * tw + n)
    S = 5
    tags = rng.integers(0, 2 ** 32, size=(n, tw), dtype=np.uint64).astype(np.uint32)
    tags &= rng.integers(0, 2 ** 32, size=(n, tw), dtype=np.uint64).astype(np.uint32)          # a quarter of the bits
    tags[:, 0] |= 1                                                        # every item has attribute 0
    need_all = np.zeros((S, tw), np.uint32)
    need_any = np.zeros((S, tw), np.uint32)
    forbid = np.zeros((S, tw), np.uint32)
    need_all[0, 0] |= 1 << 3
    need_all[0, tw - 1] |= 1 << 30                                         # two bits, in two words when tw > 1
    need_any[1, tw // 2] = 0x00F0000F                                      # segments 0, 2, 3, 4: an all-zero need_any
    forbid[2, tw - 1] = 1 << 31
    forbid[3, 0] = 1                                                       # empties the segment
    need_all[4, 0], need_any[4, tw - 1], forbid[4, tw // 2] = 1, 0xFF00, 1 << 7
    base = rng.random(n) < 0.7
    base_w = bitmap_numpy(base)
    W = (n + 31) // 32
    i32 = lambda a: upload(np.ascontiguousarray(a).view(np.int32), dev)    # noqa: E731
    for bw in (None, base_w):
        want = eref.eligibility_words(tags, need_all, need_any, forbid, bw)
        assert not want[3].any()
        if n % 32:
            assert not (want[:, -1] >> np.uint32(n % 32)).any()            # the definition's own tail
        out = torch.full((S, W), POISON_WORD, dtype=torch.int32, device=dev)
        be.eligibility_bitmaps(n=n, item_tags=i32(tags), need_all=i32(need_all), need_any=i32(need_any),
                               forbid=i32(forbid), base_allow=None if bw is None else i32(bw), out=out)
        got = out.cpu().numpy().view(np.uint32)
        assert (got == want).all(), np.argwhere(got != want)[:5]
    # absent rules are all-zero rules
    out = torch.full((S, W), POISON_WORD, dtype=torch.int32, device=dev)
    be.eligibility_bitmaps(n=n, item_tags=i32(tags), need_all=None, need_any=None, forbid=i32(forbid), base_allow=None,
                           out=out)
    assert (out.cpu().numpy().view(np.uint32) == eref.eligibility_words(tags, None, None, forbid)).all()


def test_bad_arguments_and_segment_ids_outside_the_table():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    m, n, k = 20, 200, 64
    f = factors(torch, layout, dev, m, n, k, seed=1)
    E = five_segments(n, seed=2)
    Ed = table_dev(E, dev)
    users = np.arange(m)
    # ids outside [0, S): the row has no candidates, nothing is read for it
    row_seg = np.zeros(m, np.int64)
    row_seg[3], row_seg[11] = 5, -1
    tv, ti, tc = run_topk_seg(torch, be, f, users, n, None, None, 10, dev, Ed, row_seg)
    assert tc[3] == 0 and tc[11] == 0 and (ti[[3, 11]] == -1).all() and np.isneginf(tv[[3, 11]]).all()
    ok = np.ones(m, bool)
    ok[[3, 11]] = False
    exp = run_topk(torch, be, f, users, n, None, None, 10, dev)
    assert_same((tv[ok], ti[ok], tc[ok]), tuple(a[ok] for a in exp))

    us, rs = upload(users.astype(np.int32), dev), upload(np.zeros(m, np.int32), dev)
    tvd = torch.empty(m, 10, dtype=torch.float32, device=dev)
    tid = torch.empty(m, 10, dtype=torch.int32, device=dev)
    tcd = torch.empty(m, dtype=torch.int32, device=dev)
    W = (n + 31) // 32

    def call(nseg=5, stride=W, table=Ed, seg=rs):
        return lib.als_recommend_topk_segmented(k, f["ld"], m, cptr(us), n, cptr(f["U"]), cptr(f["Z"]), cptr(f["b_u"]),
                                                cptr(f["b_i"]), cptr(f["mu"]), None, None, cptr(table), nseg, stride,
                                                cptr(seg), 10, 1, cptr(tvd), cptr(tid), cptr(tcd), None, 0, None)
    assert call() == 0
    assert call(nseg=0) == -1 and call(stride=W - 1) == -1 and call(table=None) == -1 and call(seg=None) == -1
    out = torch.empty(5, W, dtype=torch.int32, device=dev)
    tags = torch.zeros(n, 9, dtype=torch.int32, device=dev)
    for tw in (0, 9):
        assert lib.als_eligibility_bitmaps(n, tw, cptr(tags), 5, None, None, None, None, cptr(out), None) == -1
    assert lib.als_eligibility_bitmaps(n, 8, None, 5, None, None, None, None, cptr(out), None) == -1
    with pytest.raises(ValueError):
        be.recommend_topk_segmented(k=k, ld=f["ld"], users=us, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"],
                                    mu=f["mu"], seen_ptr=None, seen_idx=None, seg_allow=Ed[:, : W - 1].contiguous(),
                                    row_seg=rs, topn=10, top_val=tvd, top_idx=tid, top_cnt=tcd)
    with pytest.raises(ValueError):
        be.recommend_topk_segmented(k=k, ld=f["ld"], users=us, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"],
                                    mu=f["mu"], seen_ptr=None, seen_idx=None, seg_allow=Ed, row_seg=rs[:-1], topn=10,
                                    top_val=tvd, top_idx=tid, top_cnt=tcd)


# ---------------------------------------------------------------------------------------------- model level
def test_model_eligible_calls_on_a_fixture(monkeypatch):
    env()
    g = Golden("g4_feat_uw5")
    r, c, v = g.train
    model = model_for(g, device="cuda:0")
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=g.cfg["tol"], verbose=0)
    monkeypatch.setattr(model._eng, "REC_BATCH", 37, raising=False)        # chunks cut through the segments
    m, n = g.m, g.n
    rng = np.random.default_rng(0)
    S, A = 6, 40
    tags = rng.random((n, A)) < 0.3
    rules = dict(need_all=rng.random((S, A)) < 0.03, need_any=rng.random((S, A)) < 0.1, forbid=rng.random((S, A)) < 0.05)
    rules["need_any"][0] = False
    rules["forbid"][1] = True
    block = rng.permutation(n)[:10]
    e_tag = model.eligibility(item_tags=tags, rules=rules, filter_items=block)
    masks = eref.eligible_bool(tags, rules["need_all"], rules["need_any"], rules["forbid"],
                               ~np.isin(np.arange(n), block))
    assert (e_tag.table.cpu().numpy().view(np.uint32) == eref.table_numpy(masks)).all()
    e_mask = model.eligibility(masks)
    assert (e_mask.table == e_tag.table).all()
    assert masks.any(axis=1).sum() >= 3

    users = np.concatenate([np.arange(m)[::-1], [2, 2, 2]])
    seg = np.concatenate([rng.integers(0, S, m), [0, 3, 5]])
    for e in (e_tag, e_mask):
        for N in (10, 100):
            got = model.recommend_eligible(users, N, eligibility=e, segments=seg, features=g.features)
            assert got[0].dtype == np.int64 and got[1].dtype == np.float64
            for s in np.unique(seg):
                rows = np.nonzero(seg == s)[0]
                want = model.recommend(users[rows], N, features=g.features, items=masks[s])
                assert (got[0][rows] == want[0]).all() and (got[1][rows] == want[1]).all()

    # the all-ones single segment is recommend, element for element
    ones = model.eligibility(np.ones((1, n), dtype=bool))
    got = model.recommend_eligible(None, 20, eligibility=ones, segments=np.zeros(m, np.int64), features=g.features)
    want = model.recommend(None, 20, features=g.features)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()

    # users outside the fit
    B = 50
    R_new = np.full((B, n), np.nan)
    for b in range(B - 1):                                                 # the last row: no ratings
        R_new[b, rng.permutation(n)[: 3 + b]] = rng.integers(1, 11, 3 + b) * 0.5
    seg_new = rng.integers(0, S, B)
    got = model.recommend_new_eligible(R_new, 15, eligibility=e_tag, segments=seg_new, features=g.features)
    for s in np.unique(seg_new):
        rows = np.nonzero(seg_new == s)[0]
        want = model.recommend_new(R_new[rows], 15, features=g.features, items=masks[s])
        assert (got[0][rows] == want[0]).all() and (got[1][rows] == want[1]).all()

    # ranks: one segment per user id
    seg_of = rng.integers(0, S, m)
    P = 400
    u = rng.integers(0, m, P)
    u[:30] = 1
    it = rng.integers(0, n, P)
    got = model.rank_of_eligible(u, it, eligibility=e_tag, segments=seg_of[u], features=g.features)
    for s in np.unique(seg_of[u]):
        p = np.nonzero(seg_of[u] == s)[0]
        want = model.rank_of(u[p], it[p], features=g.features, allow_items=masks[s])
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and (a[p] == b).all()
    top, _ = model.recommend_eligible(np.arange(m), 10, eligibility=e_tag, segments=seg_of, features=g.features)
    uu, jj = np.nonzero(top >= 0)
    rank, _, _ = model.rank_of_eligible(uu, top[uu, jj], eligibility=e_tag, segments=seg_of[uu], features=g.features)
    assert (rank == jj).all()
