"""Argument checks of the sliced top-N / rank-count entry points (GPU): every C entry point of the family returns the
status include/als_hip.h documents for one malformed argument at a time, in the documented order - ALS_E_BADK before
ALS_E_BADARG, an empty batch 0 before the pointer checks, the workspace check last - and the workspace queries return
0 for malformed shapes and the documented byte count for the valid one.

The tensors are tiny and valid (k = 16, ld 16, n = 64, two batch rows, topn = 4), and every call below returns before
a kernel is launched: no case reaches a launch, so nothing is computed and nothing is compared with a reference."""
import ctypes as C
import math

import pytest

pytestmark = pytest.mark.gpu

from tests.gpu_common import env

E_BADARG, E_BADK = -1, -2
K, LD, N_CAT, ROWS, TOPN = 16, 16, 64, 2, 4
TOPK_MAX, DEEP_MAX, MAX_SLICES = 128, 1024, 64

_REC = "k ld nusers users n U Z b_u b_i mu seen_ptr seen_idx {} topn nslices top_val top_idx top_cnt {}ws wsb stream"
_RANK = ("k ld n U Z b_u b_i mu seen_ptr seen_idx {} nq q_users q_ptr q_items nt nslices t_score above n_cand ws wsb "
         "stream")
_SEG = "seg_allow nseg seg_stride_words row_seg"
_REC_PTRS = "users U Z b_u b_i mu top_val top_idx top_cnt"
_RANK_PTRS = "q_users q_ptr U Z b_u b_i mu n_cand q_items t_score above"

# fn: (argument order, batch-rows argument, catalogue-size argument, topn limit or None, required pointers, seen pair?,
#      workspace query, its arguments, its bytes with two slices, malformed arguments of this entry point alone)
ENTRY_POINTS = {
    "als_recommend_topk": (_REC.format("", ""), "nusers", "n", TOPK_MAX, _REC_PTRS, True,
                           "als_recommend_workspace_bytes", "nusers n topn nslices", 2 * ROWS * TOPN * 8, {}),
    "als_recommend_topk_masked": (_REC.format("allow", ""), "nusers", "n", TOPK_MAX, _REC_PTRS, True,
                                  "als_recommend_workspace_bytes", "nusers n topn nslices", 2 * ROWS * TOPN * 8, {}),
    "als_recommend_topk_segmented": (_REC.format(_SEG, ""), "nusers", "n", TOPK_MAX, _REC_PTRS + " seg_allow row_seg",
                                     True, "als_recommend_workspace_bytes", "nusers n topn nslices",
                                     2 * ROWS * TOPN * 8, {"nseg": (0,), "seg_stride_words": (1,)}),
    # 8 nusers (128 S + NL + S) + 64 with S = 2 slices and NL = 128
    "als_recommend_deep": (_REC.format("allow after_key", "rounds "), "nusers", "n", DEEP_MAX, _REC_PTRS, True,
                           "als_recommend_deep_workspace_bytes", "nusers n topn nslices",
                           8 * ROWS * (128 * 2 + 128 + 2) + 64, {}),
    "als_rank_count": (_RANK.format(""), "nq", "n", None, _RANK_PTRS, True,
                       "als_rank_count_workspace_bytes", "k nq nt n nslices", 2 * (ROWS + ROWS) * 4, {"nt": (-1,)}),
    "als_rank_count_masked": (_RANK.format("allow"), "nq", "n", None, _RANK_PTRS, True,
                              "als_rank_count_workspace_bytes", "k nq nt n nslices", 2 * (ROWS + ROWS) * 4,
                              {"nt": (-1,)}),
    "als_rank_count_segmented": (_RANK.format(_SEG), "nq", "n", None, _RANK_PTRS + " seg_allow row_seg", True,
                                 "als_rank_count_workspace_bytes", "k nq nt n nslices", 2 * (ROWS + ROWS) * 4,
                                 {"nt": (-1,), "nseg": (0,), "seg_stride_words": (1,)}),
    "als_similar_topk": ("k ld nq q_ids Q q_inv self_ids n T t_inv allow topn nslices top_val top_idx top_cnt ws wsb "
                         "stream", "nq", "n", TOPK_MAX, "q_ids Q q_inv T t_inv top_val top_idx top_cnt", False,
                         "als_similar_workspace_bytes", "nq n topn nslices", 2 * ROWS * TOPN * 8, {}),
    "als_audience_topk": ("k ld nq q_ids Q q_bias m U b_u mu seen_ptr seen_idx allow topn nslices top_val top_idx "
                          "top_cnt ws wsb stream", "nq", "m", TOPK_MAX,
                          "q_ids Q q_bias U b_u mu top_val top_idx top_cnt", True,
                          "als_audience_workspace_bytes", "nq m topn nslices", 2 * ROWS * TOPN * 8, {}),
    "als_group_topk": ("k ld ngroups g_ptr g_users max_members n U Z b_u b_i mu seen_ptr seen_idx allow aggregate topn "
                       "nslices top_val top_idx top_cnt ws wsb stream", "ngroups", "n", TOPK_MAX,
                       "g_ptr g_users U Z b_u b_i mu top_val top_idx top_cnt", True,
                       "als_group_workspace_bytes", "ngroups n topn nslices", 2 * ROWS * TOPN * 8,
                       {"max_members": (-1, 65), "aggregate": (-1, 3)}),
    "als_explore_topk": ("k ld nusers users n U Z b_u b_i mu W beta seen_ptr seen_idx allow topn nslices top_val "
                         "top_idx top_cnt top_lev ws wsb stream", "nusers", "n", TOPK_MAX,
                         _REC_PTRS + " W top_lev", True, "als_explore_workspace_bytes", "k nusers n topn nslices",
                         2 * ROWS * TOPN * 8, {"beta": (math.nan, math.inf)}),
}


@pytest.fixture(scope="module")
def valid():
    """The valid value of every argument name in ENTRY_POINTS; the workspace (`ws`, `wsb`) is added per entry point."""
    torch, _, _, dev = env().short
    f32 = lambda *sh: torch.zeros(*sh, dtype=torch.float32, device=dev)              # noqa: E731
    i32 = lambda *sh: torch.zeros(*sh, dtype=torch.int32, device=dev)                # noqa: E731
    i64 = lambda *sh: torch.zeros(*sh, dtype=torch.int64, device=dev)                # noqa: E731
    words = (N_CAT + 31) // 32
    v = dict(k=K, ld=LD, n=N_CAT, m=N_CAT, topn=TOPN, nslices=0, nusers=ROWS, nq=ROWS, ngroups=ROWS, nt=ROWS,
             users=i32(ROWS), q_users=i32(ROWS), q_ids=i32(ROWS), self_ids=i32(ROWS), row_seg=i32(ROWS),
             U=f32(N_CAT, LD), Z=f32(N_CAT, LD), Q=f32(N_CAT, LD), T=f32(N_CAT, LD), b_u=f32(N_CAT), b_i=f32(N_CAT),
             q_bias=f32(N_CAT), q_inv=f32(N_CAT), t_inv=f32(N_CAT),
             mu=torch.zeros(1, dtype=torch.float64, device=dev), seen_ptr=i64(N_CAT + 1), seen_idx=i32(1),
             allow=torch.full((words,), -1, dtype=torch.int32, device=dev),
             seg_allow=torch.full((1, words), -1, dtype=torch.int32, device=dev), nseg=1, seg_stride_words=words,
             after_key=None, rounds=i32(1), top_val=f32(ROWS, TOPN), top_idx=i32(ROWS, TOPN), top_cnt=i32(ROWS),
             top_lev=f32(ROWS, TOPN), q_ptr=torch.arange(ROWS + 1, dtype=torch.int64, device=dev), q_items=i32(ROWS),
             t_score=f32(ROWS), above=i32(ROWS), n_cand=i32(ROWS),
             g_ptr=torch.arange(ROWS + 1, dtype=torch.int64, device=dev), g_users=i32(ROWS), max_members=1,
             aggregate=0, W=f32(ROWS, LD, LD), beta=1.0, stream=None)       # the default stream
    v["_bytes"] = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    return v


def _c(x):
    return C.c_void_p(x.data_ptr()) if hasattr(x, "data_ptr") else x


@pytest.mark.parametrize("name", sorted(ENTRY_POINTS))
def test_malformed_arguments_return_the_documented_status(name, valid):
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    order, rows, ncat, topn_max, ptrs, has_seen, qname, qorder, two_slice_bytes, own = ENTRY_POINTS[name]
    order, ptrs, qorder = order.split(), ptrs.split(), qorder.split()
    fn, query = getattr(lib, name), getattr(lib, qname)

    def need(**kw):
        return query(*[kw.get(a, valid[a]) for a in qorder])

    # the deep call takes a workspace at every slice count; the others take none when one slice is planned
    base = dict(valid, ws=None, wsb=0)
    if name == "als_recommend_deep":
        assert need() > 0
        base.update(ws=valid["_bytes"](need()), wsb=need())
    else:
        assert need() == 0

    def call(**kw):
        return fn(*[_c(kw.get(a, base[a])) for a in order])

    assert call(k=0) == E_BADK and call(k=161) == E_BADK
    assert call(k=0, ld=LD + 16) == E_BADK                               # k is looked at before anything else
    assert call(ld=LD + 16) == E_BADARG and call(k=17) == E_BADARG       # k = 17 pads to 32
    assert call(**{ncat: 0}) == E_BADARG and call(**{ncat: 1 << 31}) == E_BADARG
    assert call(**{rows: -1}) == E_BADARG
    if topn_max is not None:
        assert call(topn=0) == E_BADARG and call(topn=topn_max + 1) == E_BADARG
    assert call(nslices=-1) == E_BADARG and call(nslices=MAX_SLICES + 1) == E_BADARG
    for arg, values in own.items():
        for bad in values:
            assert call(**{arg: bad}) == E_BADARG, (arg, bad)
    for p in ptrs:
        assert call(**{p: None}) == E_BADARG, p
    if has_seen:
        assert call(seen_idx=None) == E_BADARG and call(seen_ptr=None) == E_BADARG

    # n = 64 is two chunks of 32 items, so two slices are planned and the lists go through the workspace
    nbytes = need(nslices=2)
    assert nbytes == two_slice_bytes
    assert call(nslices=2, ws=None, wsb=0) == E_BADARG
    assert call(nslices=2, ws=None, wsb=nbytes) == E_BADARG
    assert call(nslices=2, ws=valid["_bytes"](nbytes), wsb=nbytes - 1) == E_BADARG

    # an empty batch is a no-op whatever the pointers are - but not before the shape checks
    empty = {a: None for a in order if hasattr(valid.get(a), "data_ptr")}
    empty.update({rows: 0, "ws": None, "wsb": 0})
    if "nt" in order:
        empty["nt"] = 0
    assert call(**empty) == 0
    assert call(**dict(empty, k=0)) == E_BADK and call(**dict(empty, ld=LD + 16)) == E_BADARG
    assert call(**dict(empty, nslices=-1)) == E_BADARG

    # the queries: 0 for a malformed shape, the documented count otherwise
    assert need(**{rows: 0}) == 0 and need(**{rows: -1}) == 0 and need(**{ncat: 0}) == 0 and need(nslices=-1) == 0
    if topn_max is not None:
        assert need(topn=0) == 0 and need(topn=topn_max + 1) == 0
        assert need(topn=topn_max, nslices=2) > 0
    if "k" in qorder:
        assert need(k=0, nslices=2) == 0 and need(k=161, nslices=2) == 0
    if "nt" in qorder:
        assert need(nt=-1, nslices=2) == 0
    assert need(nslices=1) == (0 if name != "als_recommend_deep" else 8 * ROWS * (128 + 128 + 1) + 64)
    assert need(nslices=MAX_SLICES) == nbytes                            # at most one slice per 32-item chunk
