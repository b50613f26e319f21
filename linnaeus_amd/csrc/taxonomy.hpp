// The taxonomy smoothing tables on the device (include/lnx.h: LNX_CE_FORM_TAXONOMY, lnx_taxonomy_rows): row t of the [C, C] soft-label
// matrix takes at most depth + 2 distinct values, so a workgroup keeps val[t, :] and the ancestor chain of t in LDS and forms S[c]
// from the chain of column c.  Used by loss.hip and hier_loss.hip.
#pragma once
#include "common.hpp"
#include "../../include/lnx.h"

// what a workgroup holds of its target row t (in LDS: indexed by a height found at run time, which a private array would spill for)
struct TaxRow {
    float val[LNX_TAX_MAX_DEPTH + 2];  // val[t, 0 .. depth + 1]
    int chain[LNX_TAX_MAX_DEPTH];      // anc[0 .. depth - 1, t]
};

// Threads 0 .. depth + 1 of the workgroup fill *s for a class t in [0, C) and every thread waits for them.  Every thread of the
// workgroup must call it (the barrier).  val == NULL leaves s->val alone (the distances need the chain only).
__device__ __forceinline__ void tax_load(TaxRow* s, const int32_t* __restrict__ anc, const float* __restrict__ val, int depth, int C, int64_t t) {
    const int i = threadIdx.x;
    if (val != nullptr && i < depth + 2) s->val[i] = val[t * (int64_t)(depth + 2) + i];
    if (i < depth) s->chain[i] = anc[(int64_t)i * C + t];
    __syncthreads();
}

// Height at which column c meets the row's class t: 0 at c == t, else the first k in 1..depth with anc[k-1, c] == anc[k-1, t] >= 0,
// or depth + 1 when the chains never meet.  Every level is loaded before any is compared (the loads are independent and `depth` is
// uniform, so their latencies overlap instead of chaining level after level); walking down from the top, the lowest match is the
// one that stays.  a[] is indexed by unrolled constants only: registers, no scratch.
__device__ __forceinline__ int tax_height(const TaxRow* s, const int32_t* __restrict__ anc, int depth, int C, int c, int64_t t) {
    int a[LNX_TAX_MAX_DEPTH];
#pragma unroll
    for (int j = 0; j < LNX_TAX_MAX_DEPTH; ++j) a[j] = j < depth ? anc[(int64_t)j * C + c] : -1;
    int k = depth + 1;
#pragma unroll
    for (int j = LNX_TAX_MAX_DEPTH - 1; j >= 0; --j)
        if (a[j] >= 0 && a[j] == s->chain[j]) k = j + 1;  // (a[j] = -1 at j >= depth: chain[j] is not read into a match)
    return c == t ? 0 : k;
}

// S[c] of row t
__device__ __forceinline__ float tax_at(const TaxRow* s, const int32_t* __restrict__ anc, int depth, int C, int c, int64_t t) {
    return s->val[tax_height(s, anc, depth, C, c, t)];
}
