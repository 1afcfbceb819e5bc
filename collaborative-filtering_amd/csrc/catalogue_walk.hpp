// What the kernels that walk the catalogue share of their walk - k_recommend (recommend.hip), k_rank_count
// (rank_eval.hip), k_similar, k_audience, k_group, k_explore: the chunk size, the slice plan, the LDS row stride, the
// lower-bound search of the seen cursors - and the epilogue of every kernel that forms a prediction (theirs,
// k_predict_dense's and k_predict_at's in predict.hip).  The host side of their entry points is topk_launch.hpp.
//
// Only what compiles to the same instructions as before lives here.  The rest of the walk - Z prefetch / staging,
// allow-bitmap scan, seen-cursor set-up, 16-entry exclusion walk, score tiles, candidate test, chunk loop - was moved
// here as well, measured and put back: as functions, member functions, lambda factories or a loop template it changed
// the register allocation of all 60 kernel instances, and on the MI355X the sliced k_recommend calls (64 ... 4096
// users, N = 10) came out 6 % slower while everything else ran 1 ... 5 % faster (DESIGN section 19,
// profiles/catalogue_walk_ab.json).  Those pieces have one text all the same: the walk_*.inc fragments next to this
// header, plain statements that a kernel #includes at the point of use, inside its body, so that the compiler reads the
// token sequence it read when they were written out and every stream stays the parent's (which lists
// the fragments and their includers; profiles/walk_text_streams.txt).  The candidate test and the chunk loop differ from
// kernel to kernel and stay in the kernels; tests/test_walk_single_text_cpu.py keeps the copies from growing back.
#pragma once
#include "als_device.hpp"

namespace walk {

constexpr int CHUNK = 32;           // items per staged chunk: two 16-item score tiles per wave
constexpr int MIN_SLICE = 2048;     // automatic slicing keeps at least this many items per slice

// ---- host: slices of the item range (grid.y)
// nslices == 0: aim at two workgroups per CU, >= MIN_SLICE items each; rows_per_wg rows share one workgroup
inline int plan_slices(int64_t nrows, int64_t rows_per_wg, int64_t n, int nslices, int max_slices) {
    const int64_t ublocks = (nrows + rows_per_wg - 1) / rows_per_wg;
    int64_t s = nslices;
    if (s == 0) {
        s = (512 + ublocks - 1) / ublocks;
        s = min(s, (n + MIN_SLICE - 1) / MIN_SLICE);
    }
    s = min(s, (int64_t)max_slices);
    s = min(s, (n + CHUNK - 1) / CHUNK);                  // every slice at least one chunk
    return (int)max(s, (int64_t)1);
}
// slice length: a whole number of chunks, so every slice but the last is full
inline int64_t slice_items(int64_t n, int nsl) {
    const int64_t nchunks = (n + CHUNK - 1) / CHUNK;
    return (nchunks + nsl - 1) / nsl * CHUNK;
}

constexpr int lds_row_stride(int KB) { return 16 * KB + 4; }    // floats per staged Z row: +16 B spreads lanes c over the banks

// ---- the epilogue of every kernel that forms a prediction from a dot product: this association, so that every score
// is bitwise the value als_predict_dense writes
__device__ __forceinline__ float score(float dot, float mu, float bu, float bi) { return dot + mu + bu + bi; }

// ---- first position in [a, e) of the ascending list whose entry is >= bound: where a seen cursor starts in a slice,
// and where it jumps to after chunks that were not scored (k_audience, k_group, k_explore; the kernels that include
// walk_seen_cursor.inc have the search written out there: section 19)
__device__ __forceinline__ int64_t lower_bound(const int32_t* __restrict__ idx, int64_t a, int64_t e, int64_t bound) {
    while (a < e) {
        const int64_t mid = a + ((e - a) >> 1);
        if (idx[mid] < bound) a = mid + 1; else e = mid;
    }
    return a;
}

}  // namespace walk
