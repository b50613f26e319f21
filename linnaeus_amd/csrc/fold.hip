// The second stage of every two-stage reduction of the deterministic mode (lnx_set_deterministic): partial sums that the first stage
// left in scratch, one row per contributor (workgroup, walker, sample row), are folded in index order and added to the destination once.
#include "common.hpp"

namespace {
// 256 threads = 16 destination elements x 16 row groups.  Row group r owns the contiguous rows [r per, (r + 1) per) and adds them in
// index order on four chains (row k of the group goes to chain k mod 4; the chains are combined pairwise); the 16 group sums meet in LDS
// and are added in group order, then to dst once.  The order depends on n alone.
__global__ __launch_bounds__(256) void fold_partials_kernel(const float* __restrict__ part, int n, int64_t stride, int64_t len, float* __restrict__ dst) {
    __shared__ float red[16][16];
    const int el = threadIdx.x & 15, r = threadIdx.x >> 4;
    const int64_t e = (int64_t)blockIdx.x * 16 + el;
    const int per = (n + 15) / 16;
    const int i0 = r * per, i1 = min(n, i0 + per);
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    if (e < len) {
        const float* src = part + e;
        int i = i0;
        for (; i + 4 <= i1; i += 4) {
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src[(int64_t)(i + j) * stride];
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] += v[j];
        }
        for (int j = 0; i < i1; ++i, ++j) t[j] += src[(int64_t)i * stride];
    }
    red[r][el] = (t[0] + t[1]) + (t[2] + t[3]);
    __syncthreads();
    if (r == 0 && e < len) {
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) a += red[k][el];
        dst[e] += a;
    }
}
}  // namespace

void launch_fold(const float* part, int n, int64_t stride, int64_t len, float* dst, hipStream_t st) {
    if (n <= 0 || len <= 0) return;
    hipLaunchKernelGGL(fold_partials_kernel, dim3((unsigned)((len + 15) / 16)), dim3(256), 0, st, part, n, stride, len, dst);
}
