// What als_recommend_deep (recommend_deep.hip) needs of recommend.hip: one scoring round of k_recommend's DEEP
// instantiations, and the slice plan of its 64-user workgroups.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace deep {

// k_recommend<KB, 4, 256, allow != NULL, DEEP> over nsl slices with per-slice topn = 128: the raw key lists go to
// part [nsl][nusers][128]; ceil [nsl][nusers] are the ceiling keys; go: NULL, or a device word that must be non-zero
// for the launch to do anything.  Returns 0, ALS_E_BADK or ALS_E_LAUNCH.
int score_round(int ld, int64_t nusers, const int32_t* users, int64_t n, int nsl, const float* U, const float* Z,
                const float* b_u, const float* b_i, const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                const uint32_t* allow, unsigned long long* part, const unsigned long long* ceil, const int32_t* go,
                hipStream_t st);

// walk::plan_slices for these workgroups: nslices == 0 is the automatic count of als_recommend_topk at topn > 32
int plan_slices(int64_t nusers, int64_t n, int nslices);

}  // namespace deep
