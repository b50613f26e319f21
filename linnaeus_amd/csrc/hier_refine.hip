// Top-down refinement of the hierarchical heads (heads/conditional_classifier_head.py:142-160, 191-224 as it was written to run; SURVEY
// F3 / F4), one launch per direction for all levels of all rows:
//     out[t][c] = base[t][c] + log(prob[parent[c]] + 1e-10),   prob = the routing probabilities over the finished row of level t + 1
// The membership matrix has at most one 1 per column, so "probs . M" is a gather through parent[]; its transpose in the backward is a
// segment sum over each parent's children (a CSR table).  Both run in O(B * sum C) instead of the O(B * C_parent * C_child) of the GEMM.
//   one workgroup of HR_THREADS owns one sample row and walks the levels (forward: coarsest to finest, backward: finest to coarsest); a
//   level's finished row goes through global memory (the same CU's vector L1 / L2) to the next level, behind a workgroup barrier.
//   Every row is walked in strides of the workgroup, so no class count has to fit anything.  Row reductions are wave butterflies
//   followed by a fixed sum over the waves' LDS slots; the segment sums run in index order in one thread.  No atomics: the same input
//   gives the same bits.
// Arithmetic is fp32 whatever the storage (the segment sums alone accumulate in fp64); a level's row enters the next level AS STORED
// (rounded to bf16 on bf16 tensors), in both directions, so the backward differentiates what the forward computed.
#include <math.h>

#include <atomic>

#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int HR_THREADS = 256;
constexpr int HR_WAVES = HR_THREADS / 64;
constexpr float HR_EPS = 1e-10f;
constexpr int HR_KEEP = 16;  // backward: strides of the workgroup whose segment sums and probabilities stay in registers between the two passes

std::atomic<int64_t> g_launches{0};  // lnx_hier_refine_launches

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < HR_WAVES; ++w) r += red[w];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < HR_WAVES; ++w) r = fmaxf(r, red[w]);
    __syncthreads();
    return r;
}
// torch.argmax order: a NaN is the largest value, ties go to the lowest index
__device__ __forceinline__ bool arg_better(float v, int j, float bv, int bj) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (vn || v == bv) return j < bj;
    return v > bv;
}
__device__ __forceinline__ int block_argmax(float v, int j, float* red, int* redi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(v, o, 64);
        const int oj = __shfl_xor(j, o, 64);
        if (arg_better(ov, oj, v, j)) {
            v = ov;
            j = oj;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = v;
        redi[threadIdx.x >> 6] = j;
    }
    __syncthreads();
    float bv = red[0];
    int bj = redi[0];
#pragma unroll
    for (int w = 1; w < HR_WAVES; ++w)
        if (arg_better(red[w], redi[w], bv, bj)) {
            bv = red[w];
            bj = redi[w];
        }
    __syncthreads();
    return bj;
}

// the routing input of parent class j: (R[j] + g[j]) / T (g = the gumbel noise or nothing)
template <typename T>
__device__ __forceinline__ float route_in(const T* __restrict__ R, const float* __restrict__ g, float temp, int j) {
    const float r = to_f(R[j]);
    return (g ? r + g[j] : r) / temp;
}

template <typename T>
__global__ __launch_bounds__(HR_THREADS) void hier_refine_fwd_kernel(const lnx_hier_refine_args a) {
    __shared__ float red[HR_WAVES];
    __shared__ int redi[HR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, nt = a.n_tasks;
    for (int t = nt - 1; t >= 0; --t) {
        const lnx_hier_refine_level& k = a.level[t];
        const int C = k.C;
        const T* __restrict__ base = static_cast<const T*>(k.base) + (int64_t)b * k.ld;
        T* out = static_cast<T*>(k.out) + (int64_t)b * k.ld;
        float* st = a.stats + ((int64_t)b * nt + t) * 2;
        if (t == nt - 1 || !k.parent) {  // pass-through: the coarsest level, or no matrix for this pair
            if (out != base)
                for (int c = tid; c < C; c += HR_THREADS) out[c] = base[c];
            if (tid == 0) st[0] = st[1] = 0.0f;
        } else {
            const lnx_hier_refine_level& p = a.level[t + 1];
            const int Cp = p.C;
            const T* R = static_cast<const T*>(p.out) + (int64_t)b * p.ld;  // written by this workgroup one level ago
            const int32_t* __restrict__ parent = k.parent;
            if (k.mode == LNX_HIER_ROUTE_HARD) {
                float bv = 0.0f;
                int bj = 0x7fffffff;
                for (int j = tid; j < Cp; j += HR_THREADS) {
                    const float v = to_f(R[j]);
                    if (bj == 0x7fffffff || arg_better(v, j, bv, bj)) {
                        bv = v;
                        bj = j;
                    }
                }
                // (a thread without an entry holds index INT_MAX and a number: any real entry beats it on the value or on the index)
                if (bj == 0x7fffffff) bv = -INFINITY;
                const int arg = block_argmax(bv, bj, red, redi);
                for (int c = tid; c < C; c += HR_THREADS) {
                    const float prob = parent[c] == arg ? 1.0f : 0.0f;
                    out[c] = from_f<T>(to_f(base[c]) + logf(prob + HR_EPS));
                }
                if (tid == 0) {
                    st[0] = to_f(R[arg]);
                    st[1] = 1.0f;
                }
            } else {
                const float temp = k.temperature;
                const float* __restrict__ g = k.mode == LNX_HIER_ROUTE_GUMBEL ? k.noise + (int64_t)b * Cp : nullptr;
                float m = -INFINITY;
                for (int j = tid; j < Cp; j += HR_THREADS) m = fmaxf(m, route_in(R, g, temp, j));
                m = block_max(m, red);
                float s = 0.0f;
                for (int j = tid; j < Cp; j += HR_THREADS) s += expf(route_in(R, g, temp, j) - m);
                s = block_sum(s, red);
                for (int c = tid; c < C; c += HR_THREADS) {
                    const int pc = parent[c];
                    const float prob = (unsigned)pc < (unsigned)Cp ? expf(route_in(R, g, temp, pc) - m) / s : 0.0f;
                    out[c] = from_f<T>(to_f(base[c]) + logf(prob + HR_EPS));
                }
                if (tid == 0) {
                    st[0] = m;
                    st[1] = s;
                }
            }
        }
        __syncthreads();  // the row is complete and visible to the whole workgroup before the level below reads it
    }
}

// S[j] = sum of the child level's G over the children of parent j, in the table's (index) order.  The one accumulator that is not
// fp32: a parent may own hundreds or thousands of children and one thread adds them one after the other; carried in fp32, a parent
// with 290 children was 2.9e-5 off where the GEMM of the torch composition (blocked sums) is 8e-6 off.  Rounded to fp32 once.
template <typename T>
__device__ __forceinline__ float segment_sum(const T* G, int Cc, const int32_t* __restrict__ start, const int32_t* __restrict__ idx, int j) {
    double s = 0.0;
    const int e = start[j + 1];
    for (int i = start[j]; i < e; ++i) {
        const int c = idx[i];
        if ((unsigned)c < (unsigned)Cc) s += (double)to_f(G[c]);
    }
    return (float)s;
}

template <typename T>
__global__ __launch_bounds__(HR_THREADS) void hier_refine_bwd_kernel(const lnx_hier_refine_args a) {
    __shared__ float red[HR_WAVES];
    const int b = blockIdx.x, tid = threadIdx.x, nt = a.n_tasks;
    for (int t = 0; t < nt; ++t) {
        const lnx_hier_refine_level& k = a.level[t];
        const int C = k.C;
        const T* __restrict__ dout = k.dout ? static_cast<const T*>(k.dout) + (int64_t)b * k.ldd : nullptr;
        T* dbase = static_cast<T*>(k.dbase) + (int64_t)b * k.ldd;
        const bool sends = t > 0 && a.level[t - 1].parent && a.level[t - 1].mode != LNX_HIER_ROUTE_HARD;
        if (!sends) {  // nothing comes up from below: G = dOut
            for (int c = tid; c < C; c += HR_THREADS) dbase[c] = dout ? dout[c] : from_f<T>(0.0f);
        } else {
            const lnx_hier_refine_level& ch = a.level[t - 1];
            const T* G = static_cast<const T*>(ch.dbase) + (int64_t)b * ch.ldd;  // written by this workgroup one level ago
            const T* __restrict__ R = static_cast<const T*>(k.out) + (int64_t)b * k.ld;
            const float temp = ch.temperature;
            const float* __restrict__ g = ch.mode == LNX_HIER_ROUTE_GUMBEL ? ch.noise + (int64_t)b * C : nullptr;
            const float* st = a.stats + ((int64_t)b * nt + (t - 1)) * 2;
            const float m = st[0], s = st[1];
            // pass 1: S, prob and the row's dot product; pass 2: dR.  What pass 1 computed for a thread's first HR_KEEP parents stays in
            // registers (static indices); parents beyond HR_KEEP strides are computed again in pass 2 (same order, same bits), so
            // nothing is sized by C
            const auto at = [&](int j, float& S, float& prob) {
                S = segment_sum(G, ch.C, ch.child_start, ch.child_idx, j);
                prob = expf(route_in(R, g, temp, j) - m) / s;
            };
            const auto store = [&](int j, float S, float prob, float dot) {
                const float dR = prob * (S / (prob + HR_EPS) - dot) / temp;
                dbase[j] = from_f<T>((dout ? to_f(dout[j]) : 0.0f) + dR);
            };
            float keepS[HR_KEEP], keepP[HR_KEEP];
            float dot = 0.0f;
#pragma unroll
            for (int u = 0; u < HR_KEEP; ++u) {
                const int j = tid + u * HR_THREADS;
                keepS[u] = keepP[u] = 0.0f;
                if (j < C) {
                    at(j, keepS[u], keepP[u]);
                    dot += keepP[u] * (keepS[u] / (keepP[u] + HR_EPS));
                }
            }
            for (int j = tid + HR_KEEP * HR_THREADS; j < C; j += HR_THREADS) {
                float S, prob;
                at(j, S, prob);
                dot += prob * (S / (prob + HR_EPS));
            }
            dot = block_sum(dot, red);
#pragma unroll
            for (int u = 0; u < HR_KEEP; ++u) {
                const int j = tid + u * HR_THREADS;
                if (j < C) store(j, keepS[u], keepP[u], dot);
            }
            for (int j = tid + HR_KEEP * HR_THREADS; j < C; j += HR_THREADS) {
                float S, prob;
                at(j, S, prob);
                store(j, S, prob, dot);
            }
        }
        __syncthreads();  // G of this level is complete before the level above sums it
    }
}

int check_args(const lnx_hier_refine_args* a, const char* who, bool bwd) {
    LNX_CHECK(a, "%s: NULL arguments", who);
    LNX_CHECK(a->dtype == 0 || a->dtype == 1, "%s: dtype=%d (0 = fp32, 1 = bf16)", who, a->dtype);
    LNX_CHECK(a->n_tasks >= 1 && a->n_tasks <= LNX_SOFTCE_MAX_TASKS, "%s: n_tasks=%d (1..%d)", who, a->n_tasks, LNX_SOFTCE_MAX_TASKS);
    LNX_CHECK(a->B > 0, "%s: B=%d", who, a->B);
    LNX_CHECK(a->stats, "%s: NULL stats", who);
    for (int t = 0; t < a->n_tasks; ++t) {
        const lnx_hier_refine_level& k = a->level[t];
        LNX_CHECK(k.C > 0, "%s: level %d has C=%d classes", who, t, k.C);
        LNX_CHECK(k.ld >= k.C, "%s: level %d has ld=%lld < C=%d", who, t, (long long)k.ld, k.C);
        LNX_CHECK(k.out, "%s: level %d has NULL out", who, t);
        if (bwd) {
            LNX_CHECK(k.dbase, "%s: level %d has NULL dbase", who, t);
            LNX_CHECK(k.ldd >= k.C, "%s: level %d has ldd=%lld < C=%d", who, t, (long long)k.ldd, k.C);
        } else {
            LNX_CHECK(k.base, "%s: level %d has NULL base", who, t);
        }
        if (t == a->n_tasks - 1 || !k.parent) continue;  // pass-through: mode, temperature, noise and the tables are not read
        LNX_CHECK(k.mode == LNX_HIER_ROUTE_SOFT || k.mode == LNX_HIER_ROUTE_HARD || k.mode == LNX_HIER_ROUTE_GUMBEL,
                  "%s: level %d has unknown routing mode %d (0 = soft, 1 = hard, 2 = gumbel)", who, t, k.mode);
        LNX_CHECK(k.temperature > 0.0f, "%s: level %d has temperature=%g (must be positive)", who, t, (double)k.temperature);
        LNX_CHECK(k.mode != LNX_HIER_ROUTE_GUMBEL || k.noise, "%s: level %d routes by gumbel and has NULL noise", who, t);
        LNX_CHECK(!bwd || (k.child_start && k.child_idx), "%s: level %d has a parent table without its CSR pair (child_start / child_idx)", who, t);
    }
    return 0;
}

}  // namespace

extern "C" int lnx_hier_refine_fwd(const lnx_hier_refine_args* a, void* stream) {
    if (int rc = check_args(a, "lnx_hier_refine_fwd", false)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == 1) hipLaunchKernelGGL(hier_refine_fwd_kernel<bf16_t>, dim3(a->B), dim3(HR_THREADS), 0, st, *a);
    else hipLaunchKernelGGL(hier_refine_fwd_kernel<float>, dim3(a->B), dim3(HR_THREADS), 0, st, *a);
    LNX_LAUNCH_CHECK();
    g_launches.fetch_add(1);
    return 0;
}

extern "C" int lnx_hier_refine_bwd(const lnx_hier_refine_args* a, void* stream) {
    if (int rc = check_args(a, "lnx_hier_refine_bwd", true)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == 1) hipLaunchKernelGGL(hier_refine_bwd_kernel<bf16_t>, dim3(a->B), dim3(HR_THREADS), 0, st, *a);
    else hipLaunchKernelGGL(hier_refine_bwd_kernel<float>, dim3(a->B), dim3(HR_THREADS), 0, st, *a);
    LNX_LAUNCH_CHECK();
    g_launches.fetch_add(1);
    return 0;
}

extern "C" int64_t lnx_hier_refine_launches(void) { return g_launches.load(); }
