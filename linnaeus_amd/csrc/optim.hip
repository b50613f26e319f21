// Multi-tensor AdamW and AdEMAMix with a fused global-norm clip for gfx950 ("optimizer + step glue").
// Replaces, for the model's parameters: torch.optim.AdamW.step (decoupled weight decay, bias correction) as built
// by linnaeus/optimizers/build.py, and the gradient-norm / clip passes of train.py:282-308
// (clip_grad_norm_: coef = min(1, max_norm / (total_norm + 1e-6)), gradients scaled by coef).
// Launches per step over a device descriptor table (one entry per parameter tensor): sum of squares of all gradients
// (partials per workgroup + a fixed-order fold; only when clipping or guarding), then the update, which reads the clip coefficient
// from that scalar.  With a non-finite guard (lnx_step_guard) the fold also decides whether the step is skipped, and every update
// kernel returns at once when it is.
#include <atomic>

#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int OPT_ELEMS = 4096;  // elements per workgroup

std::atomic<int64_t> g_launches{0};  // lnx_optim_launches

// index of the tensor that owns workgroup `block` (descriptors sorted by block_start)
__device__ __forceinline__ int find_desc_index(const lnx_adamw_desc* __restrict__ descs, int ndesc, int block) {
    int lo = 0, hi = ndesc - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (descs[mid].block_start <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ const lnx_adamw_desc& find_desc(const lnx_adamw_desc* __restrict__ descs, int ndesc, int block) {
    return descs[find_desc_index(descs, ndesc, block)];
}

// The non-finite guard (lnx_step_guard): a step kernel reads the flag the fold launch left, one 4-byte load that is uniform across the
// workgroup, and returns when it is set: a skipped step writes nothing.  The test stands behind the descriptor lookup and ahead of the
// first access to a parameter, state or gradient tensor: as the first statement of a kernel it put a branch in front of the loads of
// the other kernel arguments, which cost every launch about a microsecond, guard or no guard.
__device__ __forceinline__ bool guard_skips(const float* __restrict__ flag) { return flag != nullptr && *flag != 0.f; }

// 1 / loss scale of the step (1 without a scale): the gradient an update sees is (g * inv) * coef
__device__ __forceinline__ float guard_inv(const float* __restrict__ grad_scale) { return grad_scale != nullptr ? __fdiv_rn(1.0f, *grad_scale) : 1.0f; }

// clip coefficient from the sum of squares of the gradients as they lie in memory: total norm = sqrt(sumsq) * inv
__device__ __forceinline__ float clip_coef(const float* __restrict__ sumsq, float max_norm, float inv) {
    return sumsq != nullptr && max_norm > 0.f ? fminf(1.0f, max_norm / (sqrtf(*sumsq) * inv + 1e-6f)) : 1.0f;
}

// one partial per workgroup, folded in a fixed order by grad_sumsq_fold_kernel: the same gradients give the same bits on every
// rank and every run.  (A float atomicAdd per workgroup did not: the clip coefficient then differs in its last bits between
// data-parallel ranks that hold identical all-reduced gradients, and their parameters drift apart step by step.)
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const lnx_adamw_desc* __restrict__ descs, int ndesc, float* __restrict__ part) {
    __shared__ float red[4];
    const lnx_adamw_desc& d = find_desc(descs, ndesc, blockIdx.x);
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * OPT_ELEMS;
    const int64_t end = min(d.n, base + OPT_ELEMS);
    float s = 0.f;
    if ((reinterpret_cast<uintptr_t>(d.g) & 15) == 0) {
        for (int64_t i = base + 4 * threadIdx.x; i + 3 < end; i += 1024) {
            const float4 v = *reinterpret_cast<const float4*>(d.g + i);
            s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        const int64_t tail = base + ((end - base) & ~(int64_t)3);
        if (tail + threadIdx.x < end) {
            const float v = d.g[tail + threadIdx.x];
            s += v * v;
        }
    } else {
        for (int64_t i = base + threadIdx.x; i < end; i += 256) s += d.g[i] * d.g[i];
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// guard.flag != NULL: the fold also decides the step (out then holds two floats, the second the norm of the unscaled gradients)
__global__ __launch_bounds__(1024) void grad_sumsq_fold_kernel(const float* __restrict__ part, int n, float* __restrict__ out, const lnx_step_guard guard) {
    __shared__ float red[16];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // four independent chains per thread: loads in flight
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
        *out = t;
        if (guard.flag != nullptr) {
            out[1] = sqrtf(t) * guard_inv(guard.grad_scale);
            const bool skip = !isfinite(t) || (guard.found_inf != nullptr && *guard.found_inf != 0.f);
            *guard.flag = skip ? 1.0f : 0.0f;
            *guard.skipped += skip ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void adamw_kernel(const lnx_adamw_desc* __restrict__ descs, int ndesc, const lnx_adamw_hyper h, const float* __restrict__ sumsq,
                                                    float max_norm, const float* __restrict__ flag, const float* __restrict__ grad_scale) {
    const lnx_adamw_desc& d = find_desc(descs, ndesc, blockIdx.x);
    const int gi = d.group;
    const float lr = h.lr[gi], b1 = h.beta1[gi], b2 = h.beta2[gi], eps = h.eps[gi], wd = h.weight_decay[gi];
    const float omb1 = h.omb1[gi], omb2 = h.omb2[gi];
    const float step_size = lr / h.bias_c1[gi], inv_sqrt_bc2 = 1.0f / sqrtf(h.bias_c2[gi]);
    const float inv = guard_inv(grad_scale), coef = clip_coef(sumsq, max_norm, inv);
    if (guard_skips(flag)) return;
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * OPT_ELEMS;
    const int64_t end = min(d.n, base + OPT_ELEMS);
    auto upd = [&](float g, float& p, float& m, float& v) __attribute__((always_inline)) {
        g = (g * inv) * coef;
        p *= 1.0f - lr * wd;
        m = fmaf(b1, m, omb1 * g);
        v = fmaf(b2, v, omb2 * g * g);
        const float denom = sqrtf(v) * inv_sqrt_bc2 + eps;
        p -= step_size * (m / denom);
    };
    // 16-byte accesses, the workgroup's four rounds of loads all in flight before the first use (at 4 bytes a lane the
    // 120 M-parameter xl step took 2.0 ms for 3.4 GB: 1.65 TB/s)
    const bool vec = ((reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.g) | reinterpret_cast<uintptr_t>(d.m) | reinterpret_cast<uintptr_t>(d.v)) & 15) == 0;
    int64_t done = base;
    if (vec) {
        constexpr int R = OPT_ELEMS / 1024;
        float4 g4[R], p4[R], m4[R], v4[R];
        const int64_t full = base + ((end - base) & ~(int64_t)3);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = base + 1024 * r + 4 * threadIdx.x;
            const int64_t ic = i + 3 < full ? i : base;  // unconditional loads (a workgroup's first four elements always exist when full > base)
            if (full > base) {
                g4[r] = *reinterpret_cast<const float4*>(d.g + ic);
                p4[r] = *reinterpret_cast<const float4*>(d.p + ic);
                m4[r] = *reinterpret_cast<const float4*>(d.m + ic);
                v4[r] = *reinterpret_cast<const float4*>(d.v + ic);
            }
        }
        if (full > base) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t i = base + 1024 * r + 4 * threadIdx.x;
                if (i + 3 < full) {
                    upd(g4[r].x, p4[r].x, m4[r].x, v4[r].x);
                    upd(g4[r].y, p4[r].y, m4[r].y, v4[r].y);
                    upd(g4[r].z, p4[r].z, m4[r].z, v4[r].z);
                    upd(g4[r].w, p4[r].w, m4[r].w, v4[r].w);
                    *reinterpret_cast<float4*>(d.p + i) = p4[r];
                    *reinterpret_cast<float4*>(d.m + i) = m4[r];
                    *reinterpret_cast<float4*>(d.v + i) = v4[r];
                }
            }
        }
        done = full;
    }
    for (int64_t i = done + threadIdx.x; i < end; i += 256) {
        float p = d.p[i], m = d.m[i], v = d.v[i];
        upd(d.g[i], p, m, v);
        d.p[i] = p;
        d.m[i] = m;
        d.v[i] = v;
    }
}

// AdEMAMix (linnaeus/optimizers/ademamix.py:119-175) over the same descriptor table; slow[i] is exp_avg_slow (m3) of
// descs[i].  Per element, in the reference's order and with its quirks:
//   g = (g * inv) * coef                        (loss scale and clip coefficient, as adamw_kernel)
//   p *= 1 - lr*wd                              decoupled weight decay; the reference applies it after the moments and
//                                               before the update, which touches p only, so applying it first is the same
//   m1 = b1 m1 + (1-b1) g;  v = b2 v + (1-b2) g^2;  m3 = b3_t m3 + (1-b3_t) g
//   denom = sqrt(v) / sqrt(bc2) + eps
//   p -= (lr / bc1) * (m1 + alpha_t m3) / denom
// Quirk: the slow EMA m3 is divided by bc1 as well (it sits inside the addcdiv numerator of :175); the paper leaves m3
// uncorrected.  linnaeus trains with this form, so it is kept.  alpha_t, b3_t and 1-b3_t are per slot (they depend on
// the parameter's own step through the T_alpha_beta3 schedule) and come from the host, computed in double.
// Weight decay is written p + (-lr*wd) p, one fma, as the reference's p.add_(p, alpha=-wd*lr).
// 36 bytes per parameter: read p, g, m1, v, m3; write p, m1, v, m3.
__global__ __launch_bounds__(256) void ademamix_kernel(const lnx_adamw_desc* __restrict__ descs, float* const* __restrict__ slow, int ndesc,
                                                       const lnx_ademamix_hyper h, const float* __restrict__ sumsq, float max_norm,
                                                       const float* __restrict__ flag, const float* __restrict__ grad_scale) {
    const int di = find_desc_index(descs, ndesc, blockIdx.x);
    const lnx_adamw_desc& d = descs[di];
    float* const m3p = slow[di];
    const int gi = d.group;
    const float lr = h.lr[gi], b1 = h.beta1[gi], b2 = h.beta2[gi], eps = h.eps[gi], nlrwd = -(lr * h.weight_decay[gi]);
    const float omb1 = h.omb1[gi], omb2 = h.omb2[gi], b3 = h.beta3_t[gi], omb3 = h.omb3[gi], alpha = h.alpha_t[gi];
    const float step_size = lr / h.bias_c1[gi], sqrt_bc2 = sqrtf(h.bias_c2[gi]);
    const float inv = guard_inv(grad_scale), coef = clip_coef(sumsq, max_norm, inv);
    if (guard_skips(flag)) return;
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * OPT_ELEMS;
    const int64_t end = min(d.n, base + OPT_ELEMS);
    auto upd = [&](float g, float& p, float& m, float& v, float& s) __attribute__((always_inline)) {
        g = (g * inv) * coef;
        p = fmaf(nlrwd, p, p);
        m = fmaf(b1, m, omb1 * g);
        v = fmaf(b2, v, omb2 * g * g);
        s = fmaf(b3, s, omb3 * g);
        const float denom = sqrtf(v) / sqrt_bc2 + eps;
        p -= step_size * (fmaf(alpha, s, m) / denom);
    };
    // same access shape as adamw_kernel: 16-byte accesses, all four rounds of loads in flight before the first use; the
    // scalar loop takes tails and tensors any of whose five pointers is not 16-byte aligned (arena views at odd offsets)
    const bool vec = ((reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.g) | reinterpret_cast<uintptr_t>(d.m) | reinterpret_cast<uintptr_t>(d.v) |
                       reinterpret_cast<uintptr_t>(m3p)) & 15) == 0;
    int64_t done = base;
    if (vec) {
        constexpr int R = OPT_ELEMS / 1024;
        float4 g4[R], p4[R], m4[R], v4[R], s4[R];
        const int64_t full = base + ((end - base) & ~(int64_t)3);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = base + 1024 * r + 4 * threadIdx.x;
            const int64_t ic = i + 3 < full ? i : base;  // unconditional loads (a workgroup's first four elements always exist when full > base)
            if (full > base) {
                g4[r] = *reinterpret_cast<const float4*>(d.g + ic);
                p4[r] = *reinterpret_cast<const float4*>(d.p + ic);
                m4[r] = *reinterpret_cast<const float4*>(d.m + ic);
                v4[r] = *reinterpret_cast<const float4*>(d.v + ic);
                s4[r] = *reinterpret_cast<const float4*>(m3p + ic);
            }
        }
        if (full > base) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t i = base + 1024 * r + 4 * threadIdx.x;
                if (i + 3 < full) {
                    upd(g4[r].x, p4[r].x, m4[r].x, v4[r].x, s4[r].x);
                    upd(g4[r].y, p4[r].y, m4[r].y, v4[r].y, s4[r].y);
                    upd(g4[r].z, p4[r].z, m4[r].z, v4[r].z, s4[r].z);
                    upd(g4[r].w, p4[r].w, m4[r].w, v4[r].w, s4[r].w);
                    *reinterpret_cast<float4*>(d.p + i) = p4[r];
                    *reinterpret_cast<float4*>(d.m + i) = m4[r];
                    *reinterpret_cast<float4*>(d.v + i) = v4[r];
                    *reinterpret_cast<float4*>(m3p + i) = s4[r];
                }
            }
        }
        done = full;
    }
    for (int64_t i = done + threadIdx.x; i < end; i += 256) {
        float p = d.p[i], m = d.m[i], v = d.v[i], s = m3p[i];
        upd(d.g[i], p, m, v, s);
        d.p[i] = p;
        d.m[i] = m;
        d.v[i] = v;
        m3p[i] = s;
    }
}

// torch.optim.SGD (optimizers/build.py:89-96, 542-549, 578-585) over the same descriptor table; d.m is the momentum buffer, d.v is
// not read.  Per element, in torch's order:
//   g = (g * inv) * coef                        (loss scale and clip coefficient, as adamw_kernel)
//   g += wd p                                   coupled weight decay
//   momentum != 0:  buf = first ? g : momentum buf + (1 - dampening) g;   g = nesterov ? g + momentum buf : buf
//   p -= lr g
// `first` slots hold the parameters whose buffer does not exist yet (torch clones the gradient into it): the buffer is written, not
// read.  Slots with momentum 0 touch no buffer at all (d.m may be NULL there).  20 bytes per parameter (read p, g, buf; write p,
// buf), 16 in a first slot, 12 without momentum.  A descriptor with momentum but no buffer is left alone (the host API never builds one).
__global__ __launch_bounds__(256) void sgd_kernel(const lnx_adamw_desc* __restrict__ descs, int ndesc, const lnx_sgd_hyper h, const float* __restrict__ sumsq,
                                                  float max_norm, const float* __restrict__ flag, const float* __restrict__ grad_scale) {
    const lnx_adamw_desc& d = find_desc(descs, ndesc, blockIdx.x);
    const int gi = d.group;
    const float lr = h.lr[gi], mom = h.momentum[gi], omd = 1.0f - h.dampening[gi], wd = h.weight_decay[gi];
    const bool nesterov = h.nesterov[gi] != 0, first = h.first[gi] != 0, has_buf = mom != 0.f, rd_buf = has_buf && !first;
    if (has_buf && d.m == nullptr) return;
    const float inv = guard_inv(grad_scale), coef = clip_coef(sumsq, max_norm, inv);
    if (guard_skips(flag)) return;
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * OPT_ELEMS;
    const int64_t end = min(d.n, base + OPT_ELEMS);
    auto upd = [&](float g, float& p, float& m) __attribute__((always_inline)) {
        g = (g * inv) * coef;
        g = fmaf(wd, p, g);
        if (has_buf) {
            m = first ? g : fmaf(mom, m, omd * g);
            g = nesterov ? fmaf(mom, m, g) : m;
        }
        p = fmaf(-lr, g, p);
    };
    // same access shape as adamw_kernel: 16-byte accesses, all four rounds of loads in flight before the first use; the scalar loop
    // takes tails and tensors any of whose pointers is not 16-byte aligned (a NULL buffer counts as aligned and is never touched)
    const bool vec = ((reinterpret_cast<uintptr_t>(d.p) | reinterpret_cast<uintptr_t>(d.g) | reinterpret_cast<uintptr_t>(d.m)) & 15) == 0;
    int64_t done = base;
    if (vec) {
        constexpr int R = OPT_ELEMS / 1024;
        float4 g4[R], p4[R], m4[R];
        const int64_t full = base + ((end - base) & ~(int64_t)3);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = base + 1024 * r + 4 * threadIdx.x;
            const int64_t ic = i + 3 < full ? i : base;  // unconditional loads (a workgroup's first four elements always exist when full > base)
            m4[r] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (full > base) {
                g4[r] = *reinterpret_cast<const float4*>(d.g + ic);
                p4[r] = *reinterpret_cast<const float4*>(d.p + ic);
                if (rd_buf) m4[r] = *reinterpret_cast<const float4*>(d.m + ic);
            }
        }
        if (full > base) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t i = base + 1024 * r + 4 * threadIdx.x;
                if (i + 3 < full) {
                    upd(g4[r].x, p4[r].x, m4[r].x);
                    upd(g4[r].y, p4[r].y, m4[r].y);
                    upd(g4[r].z, p4[r].z, m4[r].z);
                    upd(g4[r].w, p4[r].w, m4[r].w);
                    *reinterpret_cast<float4*>(d.p + i) = p4[r];
                    if (has_buf) *reinterpret_cast<float4*>(d.m + i) = m4[r];
                }
            }
        }
        done = full;
    }
    for (int64_t i = done + threadIdx.x; i < end; i += 256) {
        float p = d.p[i], m = rd_buf ? d.m[i] : 0.f;
        upd(d.g[i], p, m);
        d.p[i] = p;
        if (has_buf) d.m[i] = m;
    }
}

}  // namespace

extern "C" int lnx_adamw_blocks(int64_t numel) { return (int)((numel + OPT_ELEMS - 1) / OPT_ELEMS); }

// The unsuffixed entry points are the guarded ones with a NULL guard: the same launches with NULL flag and scale pointers.
extern "C" int lnx_grad_sumsq_guarded(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, float* out, float* ws, const lnx_step_guard* guard,
                                      void* stream) {
    LNX_CHECK(descs_dev && ndesc > 0 && total_blocks > 0 && out && ws, "lnx_grad_sumsq: bad arguments (ws: total_blocks floats)");
    LNX_CHECK(guard == nullptr || (guard->flag != nullptr && guard->skipped != nullptr), "lnx_grad_sumsq_guarded: the guard needs its flag and its skipped counter");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(total_blocks), dim3(256), 0, st, descs_dev, ndesc, ws);
    hipLaunchKernelGGL(grad_sumsq_fold_kernel, dim3(1), dim3(1024), 0, st, ws, total_blocks, out, guard != nullptr ? *guard : lnx_step_guard{});
    g_launches += 2;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_grad_sumsq(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, float* out, float* ws, void* stream) {
    return lnx_grad_sumsq_guarded(descs_dev, ndesc, total_blocks, out, ws, nullptr, stream);
}

extern "C" int lnx_adamw_step_guarded(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_adamw_hyper* hyper, const float* sumsq, float max_norm,
                                      const lnx_step_guard* guard, void* stream) {
    LNX_CHECK(descs_dev && ndesc > 0 && total_blocks > 0 && hyper, "lnx_adamw_step: bad arguments");
    LNX_CHECK(hyper->ngroups > 0 && hyper->ngroups <= LNX_ADAMW_MAX_GROUPS, "lnx_adamw_step: ngroups=%d (max %d)", hyper->ngroups, LNX_ADAMW_MAX_GROUPS);
    for (int i = 0; i < hyper->ngroups; ++i)
        LNX_CHECK(hyper->bias_c1[i] > 0.f && hyper->bias_c2[i] > 0.f, "lnx_adamw_step: bias corrections of group %d must be positive (step >= 1)", i);
    LNX_CHECK(guard == nullptr || guard->flag != nullptr, "lnx_adamw_step_guarded: the guard has no flag");
    hipLaunchKernelGGL(adamw_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, ndesc, *hyper, sumsq, max_norm,
                       guard != nullptr ? (const float*)guard->flag : nullptr, guard != nullptr ? guard->grad_scale : nullptr);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_adamw_step(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_adamw_hyper* hyper, const float* sumsq, float max_norm,
                              void* stream) {
    return lnx_adamw_step_guarded(descs_dev, ndesc, total_blocks, hyper, sumsq, max_norm, nullptr, stream);
}

extern "C" int lnx_ademamix_step_guarded(const lnx_adamw_desc* descs_dev, float* const* slow_dev, int ndesc, int total_blocks, const lnx_ademamix_hyper* hyper,
                                         const float* sumsq, float max_norm, const lnx_step_guard* guard, void* stream) {
    LNX_CHECK(descs_dev && slow_dev && ndesc > 0 && total_blocks > 0 && hyper, "lnx_ademamix_step: bad arguments");
    LNX_CHECK(hyper->ngroups > 0 && hyper->ngroups <= LNX_ADAMW_MAX_GROUPS, "lnx_ademamix_step: ngroups=%d (max %d)", hyper->ngroups, LNX_ADAMW_MAX_GROUPS);
    for (int i = 0; i < hyper->ngroups; ++i)
        LNX_CHECK(hyper->bias_c1[i] > 0.f && hyper->bias_c2[i] > 0.f, "lnx_ademamix_step: bias corrections of slot %d must be positive (step >= 1)", i);
    LNX_CHECK(guard == nullptr || guard->flag != nullptr, "lnx_ademamix_step_guarded: the guard has no flag");
    hipLaunchKernelGGL(ademamix_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, slow_dev, ndesc, *hyper, sumsq, max_norm,
                       guard != nullptr ? (const float*)guard->flag : nullptr, guard != nullptr ? guard->grad_scale : nullptr);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_ademamix_step(const lnx_adamw_desc* descs_dev, float* const* slow_dev, int ndesc, int total_blocks, const lnx_ademamix_hyper* hyper,
                                 const float* sumsq, float max_norm, void* stream) {
    return lnx_ademamix_step_guarded(descs_dev, slow_dev, ndesc, total_blocks, hyper, sumsq, max_norm, nullptr, stream);
}

extern "C" int lnx_sgd_step_guarded(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_sgd_hyper* hyper, const float* sumsq, float max_norm,
                                    const lnx_step_guard* guard, void* stream) {
    LNX_CHECK(descs_dev != nullptr && hyper != nullptr, "lnx_sgd_step: NULL descriptor table or hyper-parameter table");
    LNX_CHECK(ndesc > 0, "lnx_sgd_step: ndesc=%d (must be positive)", ndesc);
    LNX_CHECK(total_blocks > 0, "lnx_sgd_step: total_blocks=%d (must be positive)", total_blocks);
    LNX_CHECK(hyper->ngroups > 0 && hyper->ngroups <= LNX_ADAMW_MAX_GROUPS, "lnx_sgd_step: ngroups=%d (1..%d)", hyper->ngroups, LNX_ADAMW_MAX_GROUPS);
    for (int i = 0; i < hyper->ngroups; ++i) {
        LNX_CHECK(hyper->lr[i] >= 0.f, "lnx_sgd_step: negative lr in slot %d", i);
        LNX_CHECK(hyper->momentum[i] >= 0.f, "lnx_sgd_step: negative momentum in slot %d", i);
        LNX_CHECK(hyper->weight_decay[i] >= 0.f, "lnx_sgd_step: negative weight_decay in slot %d", i);
        LNX_CHECK(!hyper->nesterov[i] || (hyper->momentum[i] > 0.f && hyper->dampening[i] == 0.f),
                  "lnx_sgd_step: nesterov in slot %d needs a momentum above zero and zero dampening", i);
    }
    LNX_CHECK(guard == nullptr || guard->flag != nullptr, "lnx_sgd_step_guarded: the guard has no flag");
    hipLaunchKernelGGL(sgd_kernel, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, descs_dev, ndesc, *hyper, sumsq, max_norm,
                       guard != nullptr ? (const float*)guard->flag : nullptr, guard != nullptr ? guard->grad_scale : nullptr);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_sgd_step(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_sgd_hyper* hyper, const float* sumsq, float max_norm,
                            void* stream) {
    return lnx_sgd_step_guarded(descs_dev, ndesc, total_blocks, hyper, sumsq, max_norm, nullptr, stream);
}

extern "C" int64_t lnx_optim_launches(void) { return g_launches.load(); }
