// Fold of a split row's partial slots into its first slot (k_sum_slots, k_sum_slots_f64).
//
// Every element of slot 0 becomes  acc = first; acc += slot 1; ... acc += slot nslots-1  - ascending slot order, one
// round-to-nearest add per slot: bitwise the sum of a thread that walks the slots one by one.  Only the loads are
// arranged differently: a thread owns one 16-byte vector V (f32x4 / f64x2; the components are independent chains,
// each in slot order), takes the slots in blocks of B, and has the loads of the next block in flight while the add
// chain of the current one runs, so the chain waits for one memory round trip per B slots instead of one per slot.
//
// The (nslots - 1) % B slots that fill no block come FIRST (slots 1 ... rem), through the same load<CNT> / add<CNT>
// pair with CNT = rem chosen by a switch: a per-load "if (j < cnt)" inside one block makes the compiler branch
// around every load and wait for each on its own.  The full blocks alternate between two register sets.
#pragma once
#include "als_device.hpp"

#ifndef ALS_SLOT_FOLD_BLOCK
#define ALS_SLOT_FOLD_BLOCK 16      // slots per block (8, 16 or 32; DESIGN section 4, "Slot fold"); the tests read it
#endif

namespace slot_fold {

typedef double f64x2 __attribute__((ext_vector_type(2)));

// slots 1 ... are read once: nontemporal, they need not stay in any cache
template <int CNT, typename V>
__device__ __forceinline__ void load_block(V (&t)[ALS_SLOT_FOLD_BLOCK], const V* __restrict__ p, size_t stride) {
#pragma unroll
    for (int j = 0; j < CNT; ++j) t[j] = __builtin_nontemporal_load(p + j * stride);
}

template <int CNT, typename V>
__device__ __forceinline__ void add_block(V& acc, const V (&t)[ALS_SLOT_FOLD_BLOCK]) {
    constexpr int NC = sizeof(V) / sizeof(acc[0]);
    __builtin_amdgcn_sched_barrier(0);          // the loads issued so far stay ahead of this chain
#pragma unroll
    for (int j = 0; j < CNT; ++j)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += t[j][c];
}

template <int CNT, typename V>
__device__ __forceinline__ void fold_short(V& acc, const V* __restrict__ p, size_t stride) {
    V t[ALS_SLOT_FOLD_BLOCK];
    load_block<CNT>(t, p, stride);
    add_block<CNT>(acc, t);
}

// slots 1 ... n (n < B, wave-uniform) at p: one straight-line load<n> / add<n> pair per value of n
template <typename V>
__device__ __forceinline__ void fold_rem(V& acc, const V* __restrict__ p, size_t stride, int n) {
    constexpr int B = ALS_SLOT_FOLD_BLOCK;
    static_assert(B == 8 || B == 16 || B == 32, "the switch below covers 1 ... B - 1");
    switch (n) {
#define ALS_FOLD_CASE(r) case r: if (r < B) fold_short<(r < B ? r : 1)>(acc, p, stride); break;
        ALS_FOLD_CASE(1) ALS_FOLD_CASE(2) ALS_FOLD_CASE(3) ALS_FOLD_CASE(4) ALS_FOLD_CASE(5) ALS_FOLD_CASE(6)
        ALS_FOLD_CASE(7) ALS_FOLD_CASE(8) ALS_FOLD_CASE(9) ALS_FOLD_CASE(10) ALS_FOLD_CASE(11) ALS_FOLD_CASE(12)
        ALS_FOLD_CASE(13) ALS_FOLD_CASE(14) ALS_FOLD_CASE(15) ALS_FOLD_CASE(16) ALS_FOLD_CASE(17) ALS_FOLD_CASE(18)
        ALS_FOLD_CASE(19) ALS_FOLD_CASE(20) ALS_FOLD_CASE(21) ALS_FOLD_CASE(22) ALS_FOLD_CASE(23) ALS_FOLD_CASE(24)
        ALS_FOLD_CASE(25) ALS_FOLD_CASE(26) ALS_FOLD_CASE(27) ALS_FOLD_CASE(28) ALS_FOLD_CASE(29) ALS_FOLD_CASE(30)
        ALS_FOLD_CASE(31)
#undef ALS_FOLD_CASE
        default: break;
    }
}

// The sum of the thread's vector over slots 0 ... nslots-1 (nslots >= 1, wave-uniform); w0: its vector of slot 0,
// stride: vectors per slot.  ZERO_FIRST: the chain starts as 0 + slot 0 (the fp32 kernel's, which turns a -0 into +0).
template <bool ZERO_FIRST, typename V>
__device__ __forceinline__ V fold(const V* __restrict__ w0, size_t stride, int nslots) {
    constexpr int B = ALS_SLOT_FOLD_BLOCK;
    const int rem = (nslots - 1) % B;
    int nfull = (nslots - 1) / B;
    const V* p = w0 + stride;                   // slot 1
    const V* pf = p + rem * stride;             // first full block
    const V first = w0[0];                      // plain load: the sum is stored here and read again at once
    V acc;
    if (nfull == 0) {
        acc = ZERO_FIRST ? V(0) + first : first;
        fold_rem(acc, p, stride, rem);
        return acc;
    }
    // Both register sets are loaded without a condition of their own: a load that may or may not have been issued
    // makes the compiler wait for everything at the next use of any loaded value.
    V a[B], b[B];
    load_block<B>(a, pf, stride);
    __builtin_amdgcn_sched_barrier(0);
    acc = ZERO_FIRST ? V(0) + first : first;
    fold_rem(acc, p, stride, rem);
    // a holds the block at pf; the last one or two blocks are peeled
    while (nfull > 2) {
        load_block<B>(b, pf + (size_t)B * stride, stride);
        add_block<B>(acc, a);
        load_block<B>(a, pf + (size_t)(2 * B) * stride, stride);
        add_block<B>(acc, b);
        pf += (size_t)(2 * B) * stride;
        nfull -= 2;
    }
    if (nfull == 2) {
        load_block<B>(b, pf + (size_t)B * stride, stride);
        add_block<B>(acc, a);
        add_block<B>(acc, b);
    } else {
        add_block<B>(acc, a);
    }
    return acc;
}

}  // namespace slot_fold
