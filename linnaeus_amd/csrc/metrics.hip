// Validation metrics on the device (utils/metrics/tracker.py:609-937 MetricsTracker._update_phase_batch, chain_accuracy.py:143-166,299-344):
// one launch per batch adds every counter of every task to the caller's int64 counts[] / double sums[] tables (layout: include/lnx.h).
//   workgroups 0 .. ceil(B / 4) - 1   four waves, ONE WAVE PER SAMPLE over all tasks.  A task's verdict needs no sort: the target's rank
//                                     is the number of entries of the row that come before it in (value descending, index ascending, NaN
//                                     first) order, so the wave reads the row once, every lane counts, one wave_sum gives the rank, and
//                                     the chain flags stay in registers across the tasks.  Counters meet in LDS and leave as one integer
//                                     atomic per non-zero counter per workgroup (integers: exact in any order).
//   the last workgroup                the loss sums: all B losses of every task in double, each thread a fixed stride, a fixed LDS tree --
//                                     the only writer of sums[], so the same input gives the same bits and no workspace is needed.
#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int MT_WAVES = 4;                                                              // samples per workgroup
constexpr int MT_NCTR = LNX_METRICS_HEAD + LNX_METRICS_TASK_STRIDE * LNX_SOFTCE_MAX_TASKS;  // counters in front of the subset bins

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// does entry (v, j) come before the target's (xt, tj)?  value descending, index ascending, NaN above every number
__device__ __forceinline__ int before(float v, int j, float xt, int tj, bool t_nan) {
    const bool v_nan = v != v;
    const bool first = j < tj;
    return (v_nan ? (!t_nan || first) : (!t_nan && (v > xt || (v == xt && first)))) ? 1 : 0;
}

__device__ __forceinline__ float bf16_bits_to_f(uint32_t b) { return __uint_as_float(b << 16); }

// entries of row[0, C) that come before entry tj, counted by the 64 lanes of one wave (the caller sums the lanes)
template <typename T>
__device__ __forceinline__ int count_before(const T* __restrict__ row, int C, int tj, int lane) {
    constexpr int EPV = TT<T>::EPV;
    const float xt = to_f(row[tj]);
    const bool t_nan = xt != xt;
    int n = 0, done = 0;
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {  // 16-byte loads over the aligned body of the row (wave-uniform branch)
        const int nvec = C / EPV;
        for (int v = lane; v < nvec; v += 64) {
            const uint4 raw = ld16(row + (int64_t)v * EPV);
            const int j0 = v * EPV;
            if constexpr (EPV == 4) {
                n += before(__uint_as_float(raw.x), j0, xt, tj, t_nan) + before(__uint_as_float(raw.y), j0 + 1, xt, tj, t_nan) +
                     before(__uint_as_float(raw.z), j0 + 2, xt, tj, t_nan) + before(__uint_as_float(raw.w), j0 + 3, xt, tj, t_nan);
            } else {
                const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    n += before(bf16_bits_to_f(w[k] & 0xffffu), j0 + 2 * k, xt, tj, t_nan) + before(bf16_bits_to_f(w[k] >> 16), j0 + 2 * k + 1, xt, tj, t_nan);
            }
        }
        done = nvec * EPV;
    }
    for (int j = done + lane; j < C; j += 64) n += before(to_f(row[j]), j, xt, tj, t_nan);
    return n;
}

__global__ __launch_bounds__(64 * MT_WAVES) void metrics_update_kernel(const lnx_metrics_args a) {
    __shared__ int ctr[MT_NCTR];
    __shared__ double red[64 * MT_WAVES];
    const int T = a.n_tasks, tid = threadIdx.x;

    if (blockIdx.x == gridDim.x - 1) {  // ---- the loss sums
        for (int t = 0; t < T; ++t) {
            const lnx_metrics_task& k = a.task[t];
            if (!k.loss) continue;  // (uniform)
            double s_null = 0.0, s_non = 0.0;
            for (int b = tid; b < a.B; b += 64 * MT_WAVES) {
                const bool null = k.is_null ? k.is_null[b] != 0 : k.target[b] == 0;
                const double l = (double)k.loss[b];
                if (null) s_null += l;
                else s_non += l;
            }
            double out[2];
#pragma unroll
            for (int which = 0; which < 2; ++which) {
                __syncthreads();
                red[tid] = which ? s_non : s_null;
                __syncthreads();
                for (int w = 32 * MT_WAVES; w > 0; w >>= 1) {
                    if (tid < w) red[tid] += red[tid + w];
                    __syncthreads();
                }
                out[which] = red[0];
            }
            if (tid == 0) {
                double* s = a.sums + LNX_METRICS_SUM(t);
                s[LNX_METRICS_SUM_NULL_LOSS] += out[0];
                s[LNX_METRICS_SUM_NONNULL_LOSS] += out[1];
                s[LNX_METRICS_SUM_LOSS] += out[0] + out[1];
                atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + LNX_METRICS_TASK(t) + LNX_METRICS_LOSS_N), (unsigned long long)a.B);
            }
        }
        return;
    }

    // ---- one wave per sample
    for (int i = tid; i < MT_NCTR; i += 64 * MT_WAVES) ctr[i] = 0;
    __syncthreads();
    const int lane = tid & 63;
    const int b = blockIdx.x * MT_WAVES + (tid >> 6);
    if (b < a.B) {  // (wave-uniform)
        bool prefix_ok = true, any_non_null = false, partial_ok = false;
        unsigned right_mask = 0;
        for (int t = 0; t < T; ++t) {
            const lnx_metrics_task& k = a.task[t];
            const int64_t tg = k.target[b];
            int rank = 3;
            if (tg >= 0 && tg < k.C) {
                const int n = a.dtype == 1 ? count_before(static_cast<const bf16_t*>(k.logits) + (int64_t)b * k.ld, k.C, (int)tg, lane)
                                           : count_before(static_cast<const float*>(k.logits) + (int64_t)b * k.ld, k.C, (int)tg, lane);
                rank = wave_sum_i(n);
            }
            const bool c1 = rank == 0, c3 = k.C < 3 ? c1 : rank < 3;
            prefix_ok = prefix_ok && c1;
            if (tg != 0) {
                any_non_null = true;
                partial_ok = prefix_ok;
            }
            if (c1) right_mask |= 1u << t;
            if (lane == 0) {
                int* c = ctr + LNX_METRICS_TASK(t);
                const bool null = k.is_null ? k.is_null[b] != 0 : tg == 0;
                atomicAdd(c + LNX_METRICS_N, 1);
                if (c1) atomicAdd(c + LNX_METRICS_CORRECT1, 1);
                if (c3) atomicAdd(c + LNX_METRICS_CORRECT3, 1);
                atomicAdd(c + (null ? LNX_METRICS_NULL_N : LNX_METRICS_NONNULL_N), 1);
                if (c1) atomicAdd(c + (null ? LNX_METRICS_NULL_CORRECT1 : LNX_METRICS_NONNULL_CORRECT1), 1);
            }
        }
        if (lane == 0) {
            atomicAdd(ctr + LNX_METRICS_CHAIN_N, 1);
            if (prefix_ok) atomicAdd(ctr + LNX_METRICS_CHAIN_CORRECT, 1);
            if (any_non_null) atomicAdd(ctr + LNX_METRICS_PARTIAL_N, 1);
            if (any_non_null && partial_ok) atomicAdd(ctr + LNX_METRICS_PARTIAL_CORRECT, 1);
        }
        // subset bins: lane 2t adds n, lane 2t + 1 adds correct1 of task t (bins are many and sparse: straight to the table)
        for (int s = 0; s < 2; ++s) {
            if (!a.subset_ids[s]) continue;
            const int64_t id = a.subset_ids[s][b];
            if (id < 0 || id >= a.n_bins[s]) {
                if (lane == 0) atomicAdd(ctr + LNX_METRICS_SUBSET_OOR + s, 1);
                continue;
            }
            const int t = lane >> 1;
            if (t < T && (!(lane & 1) || ((right_mask >> t) & 1u))) {
                int64_t* dst = a.counts + LNX_METRICS_SUBSET(T, a.n_bins[0], s) + 2 * ((int64_t)t * a.n_bins[s] + id) + (lane & 1);
                atomicAdd(reinterpret_cast<unsigned long long*>(dst), 1ull);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < LNX_METRICS_TASK(T); i += 64 * MT_WAVES)
        if (ctr[i]) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts + i), (unsigned long long)ctr[i]);
}

}  // namespace

extern "C" int lnx_metrics_table_sizes(int n_tasks, int n_bins0, int n_bins1, int64_t* n_counts, int64_t* n_sums) {
    LNX_CHECK(n_tasks >= 1 && n_tasks <= LNX_SOFTCE_MAX_TASKS, "lnx_metrics_table_sizes: n_tasks=%d (1..%d)", n_tasks, LNX_SOFTCE_MAX_TASKS);
    LNX_CHECK(n_bins0 >= 0 && n_bins1 >= 0 && n_counts && n_sums, "lnx_metrics_table_sizes: negative bin count or NULL output");
    *n_counts = LNX_METRICS_SUBSET(n_tasks, n_bins0, 1) + 2 * (int64_t)n_tasks * n_bins1;
    *n_sums = LNX_METRICS_SUM(n_tasks);
    return 0;
}

extern "C" int lnx_metrics_update(const lnx_metrics_args* a, void* stream) {
    LNX_CHECK(a, "lnx_metrics_update: NULL arguments");
    LNX_CHECK(a->n_tasks >= 1 && a->n_tasks <= LNX_SOFTCE_MAX_TASKS, "lnx_metrics_update: n_tasks=%d (1..%d)", a->n_tasks, LNX_SOFTCE_MAX_TASKS);
    LNX_CHECK(a->counts && a->sums, "lnx_metrics_update: NULL counts / sums table");
    LNX_CHECK(a->dtype == 0 || a->dtype == 1, "lnx_metrics_update: dtype=%d (0 = fp32, 1 = bf16)", a->dtype);
    LNX_CHECK(a->B >= 0, "lnx_metrics_update: B=%d", a->B);
    for (int t = 0; t < a->n_tasks; ++t) {
        const lnx_metrics_task& k = a->task[t];
        LNX_CHECK(k.C >= 1, "lnx_metrics_update: task %d has C=%d classes", t, k.C);
        LNX_CHECK(k.ld >= k.C, "lnx_metrics_update: task %d has ld=%lld < C=%d", t, (long long)k.ld, k.C);
        LNX_CHECK(k.logits && k.target, "lnx_metrics_update: task %d has NULL logits / target", t);
    }
    for (int s = 0; s < 2; ++s)
        LNX_CHECK(a->subset_ids[s] ? a->n_bins[s] >= 1 : a->n_bins[s] == 0, "lnx_metrics_update: subset type %d has n_bins=%d (>= 1 with ids, 0 without)", s,
                  a->n_bins[s]);
    if (a->B == 0) return 0;
    hipLaunchKernelGGL(metrics_update_kernel, dim3(cdiv(a->B, MT_WAVES) + 1), dim3(64 * MT_WAVES), 0, (hipStream_t)stream, *a);
    LNX_LAUNCH_CHECK();
    return 0;
}
