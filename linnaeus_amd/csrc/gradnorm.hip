// GradNorm task weighting on the device (loss/gradnorm.py GradNormModule.measure_and_update, loss/gradient_weighting.py:367-880).
// Two pieces the host glue (linnaeus_amd.loss.GradientWeighting) chains behind the per-task backward passes:
//   lnx_gradnorm_sumsq   per task, the sum of squares of the backbone slices of that task's gradient arena, with the block shape and
//                        the two-pass fixed-order fold of optim.hip's grad_sumsq kernels (same gradients -> same bits on every rank);
//                        all tasks' arenas in one launch when they are laid out at a fixed stride
//   lnx_gradnorm_update  one workgroup: initial losses, average norm, targets, the weight update and the metrics vector
#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int GN_ELEMS = 4096;  // elements per workgroup (== optim.hip's OPT_ELEMS: lnx_adamw_blocks counts the table's workgroups)

__device__ __forceinline__ int find_desc_index(const lnx_adamw_desc* __restrict__ descs, int ndesc, int block) {
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].block_start <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// blockIdx.y = task: its gradients are the table's at an offset of task_stride floats
__global__ __launch_bounds__(256) void gradnorm_sumsq_kernel(const lnx_adamw_desc* __restrict__ descs, int ndesc, int64_t task_stride,
                                                             float* __restrict__ part) {
    __shared__ float red[4];
    const lnx_adamw_desc& d = descs[find_desc_index(descs, ndesc, blockIdx.x)];
    const float* __restrict__ g = d.g + (int64_t)blockIdx.y * task_stride;
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * GN_ELEMS;
    const int64_t end = min(d.n, base + GN_ELEMS);
    float s = 0.f;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
        for (int64_t i = base + 4 * threadIdx.x; i + 3 < end; i += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(g + i);
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        const int64_t tail = base + ((end - base) & ~(int64_t)3);
        if (tail + threadIdx.x < end) {
            const float v = g[tail + threadIdx.x];
            s += v * v;
        }
    } else {
        for (int64_t i = base + threadIdx.x; i < end; i += 256) s += g[i] * g[i];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// blockIdx.x = task: fold its n partials in a fixed order; sumsq[t] (optional) and norm[t] = sqrt(sumsq[t])
__global__ __launch_bounds__(1024) void gradnorm_fold_kernel(const float* __restrict__ parts, int n, float* __restrict__ sumsq, float* __restrict__ norm) {
    __shared__ float red[16];
    const float* __restrict__ part = parts + (int64_t)blockIdx.x * n;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = threadIdx.x;
    for (; i + 3 * 1024 < n; i += 4 * 1024) {
        s0 += part[i];
        s1 += part[i + 1024];
        s2 += part[i + 2048];
        s3 += part[i + 3072];
    }
    for (; i < n; i += 1024) s0 += part[i];
    float s = wave_sum((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k];
        if (sumsq) sumsq[blockIdx.x] = t;
        norm[blockIdx.x] = sqrtf(t);
    }
}

// T <= LNX_MAX_TASKS scalars: one lane does the arithmetic in the reference's order (everything in sorted-task order)
__global__ __launch_bounds__(64) void gradnorm_update_kernel(const lnx_gradnorm_args a) {
    if (threadIdx.x != 0) return;
    const int T = a.T;
    const float Tf = (float)T;
    float loss[LNX_MAX_TASKS], target[LNX_MAX_TASKS], ratio[LNX_MAX_TASKS], w[LNX_MAX_TASKS];
    for (int i = 0; i < T; ++i) loss[i] = a.loss_sum[i] / fmaxf(a.count[i], 1.0f);  // Σ loss over valid rows / max(Σ valid, 1)
    if (a.alpha > 0.f && *a.initted == 0) {  // gradnorm.py:197-211: the first call with alpha > 0 fixes L_i(0)
        for (int i = 0; i < T; ++i) a.initial_losses[i] = a.init_loss ? a.init_loss[i] : loss[i];
        *a.initted = 1;
    }
    float gsum = 0.f;
    for (int i = 0; i < T; ++i) gsum += a.norm[i];
    const float g_avg = gsum / Tf;
    if (a.alpha > 0.f) {
        float rsum = 0.f;
        for (int i = 0; i < T; ++i) {
            ratio[i] = loss[i] / fmaxf(a.initial_losses[i], 1e-8f);
            rsum += ratio[i];
        }
        const float k = Tf / fmaxf(rsum, 1e-8f);
        for (int i = 0; i < T; ++i) {
            ratio[i] = ratio[i] * k;
            target[i] = g_avg * powf(ratio[i], a.alpha);
        }
    } else {
        for (int i = 0; i < T; ++i) {
            ratio[i] = 1.0f;
            target[i] = g_avg;
        }
    }
    float wsum = 0.f;
    for (int i = 0; i < T; ++i) {
        w[i] = a.weights[i];
        if (!(target[i] < 1e-8f)) w[i] = w[i] * (a.norm[i] / target[i]);  // a target below 1e-8 leaves the weight as it is
        wsum += w[i];
    }
    const float kw = Tf / fmaxf(wsum, 1e-8f);
    for (int i = 0; i < T; ++i) a.weights[i] = w[i] * kw;
    if (a.metrics) {
        float* m = a.metrics;
        m[0] = g_avg;
        for (int i = 0; i < T; ++i) {
            m[1 + i] = loss[i];
            m[1 + T + i] = a.norm[i];
            m[1 + 2 * T + i] = target[i];
            m[1 + 3 * T + i] = w[i] * kw;
            m[1 + 4 * T + i] = ratio[i];
        }
    }
}

}  // namespace

extern "C" int lnx_gradnorm_sumsq(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, int ntasks, int64_t task_stride, float* sumsq, float* norm,
                                  float* ws, void* stream) {
    LNX_CHECK(descs_dev && ndesc > 0 && total_blocks > 0 && norm && ws, "lnx_gradnorm_sumsq: bad arguments (ws: ntasks * total_blocks floats)");
    LNX_CHECK(ntasks >= 1 && ntasks <= LNX_MAX_TASKS, "lnx_gradnorm_sumsq: ntasks=%d (1..%d)", ntasks, LNX_MAX_TASKS);
    LNX_CHECK(ntasks == 1 || task_stride > 0, "lnx_gradnorm_sumsq: task_stride must be positive for several tasks");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gradnorm_sumsq_kernel, dim3(total_blocks, ntasks), dim3(256), 0, st, descs_dev, ndesc, task_stride, ws);
    hipLaunchKernelGGL(gradnorm_fold_kernel, dim3(ntasks), dim3(1024), 0, st, ws, total_blocks, sumsq, norm);
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_gradnorm_update(const lnx_gradnorm_args* a, void* stream) {
    LNX_CHECK(a && a->T >= 1 && a->T <= LNX_MAX_TASKS, "lnx_gradnorm_update: T must be 1..%d", LNX_MAX_TASKS);
    LNX_CHECK(a->norm && a->loss_sum && a->count && a->weights && a->initial_losses && a->initted, "lnx_gradnorm_update: null operand");
    LNX_CHECK(a->alpha >= 0.f, "lnx_gradnorm_update: alpha must be >= 0");
    hipLaunchKernelGGL(gradnorm_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *a);
    LNX_LAUNCH_CHECK();
    return 0;
}
