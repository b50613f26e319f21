// Predictions on the device (inference/handler.py:186-228 LinnaeusInferenceHandler.predict, inference/postprocessing.py:14-171
// enforce_hierarchical_consistency): one launch per batch turns the logits of every task into the final top-k (id, probability) lists.
//   workgroups of four waves, ONE WAVE PER SAMPLE, walking the sample's tasks from the coarsest to the finest; the "consistent node" of
//   the task above stays in a register.  A row is read once.  Every entry becomes one 64-bit key
//       (order-preserving image of the value) << 32 | ~index
//   so that "value descending, then index ascending, NaN above every number" (the order of metrics.hip) is one unsigned compare, and the
//   key gives the value back.  Each lane keeps the KC best keys of its share of the row, sorted, in registers (static indices only), and
//   an online max / sum of exponentials.  The 64 lists are merged by n rounds of a 64-lane arg-best with __shfl_xor: the lane that owns
//   the winner pops it, lane r keeps the r-th winner.  The max / sum pairs merge with the usual rescaling, the operands always in lane
//   order, so both partners of a butterfly step compute the same bits.  Lanes 0 .. K-1 write the outputs.  No atomics, no LDS, no
//   workspace.
#include <math.h>

#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int PD_WAVES = 4;  // samples per workgroup

// float bits -> a key that grows with the value; -0 and +0 share one key, every NaN takes the largest.  Never 0 for a real entry
// (the smallest, -inf, is 0x007fffff), so a zero 64-bit key means "empty".
__device__ __forceinline__ uint32_t order_key(uint32_t bits) {
    if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;  // NaN
    if ((bits & 0x7fffffffu) == 0u) return 0x80000000u;          // +-0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

template <int KC>
struct Lane {
    uint64_t best[KC];  // sorted, largest first; 0 = empty
    float m, s;         // running max of the numbers seen and sum of exp(x - m) over them (a NaN is left out: the row's top-1 tells)

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < KC; ++j) best[j] = 0;
        m = -INFINITY;
        s = 0.0f;
    }
    __device__ __forceinline__ void push(uint32_t bits, int j) {
        const float x = __uint_as_float(bits);
        if (x > m) {
            s = s * expf(m - x) + 1.0f;
            m = x;
        } else if (x > -INFINITY) {
            s += expf(x - m);
        }
        const uint64_t k = ((uint64_t)order_key(bits) << 32) | (uint32_t)(0xffffffffu - (uint32_t)j);
        if (k > best[KC - 1]) {
#pragma unroll
            for (int i = KC - 1; i > 0; --i) best[i] = k > best[i - 1] ? best[i - 1] : (k > best[i] ? k : best[i]);
            best[0] = k > best[0] ? k : best[0];
        }
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int i = 0; i + 1 < KC; ++i) best[i] = best[i + 1];
        best[KC - 1] = 0;
    }
};

template <int KC, typename T>
__device__ __forceinline__ void scan_row(Lane<KC>& ln, const T* __restrict__ row, int C, int lane) {
    constexpr int EPV = TT<T>::EPV;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {  // 16-byte loads over the aligned body of the row (wave-uniform branch)
        const int nvec = C / EPV;
        for (int v = lane; v < nvec; v += 64) {
            const uint4 raw = ld16(row + (int64_t)v * EPV);
            const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
            const int j0 = v * EPV;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if constexpr (EPV == 4) {
                    ln.push(w[k], j0 + k);
                } else {  // bf16 -> float is exact: the bits move up
                    ln.push(w[k] << 16, j0 + 2 * k);
                    ln.push(w[k] & 0xffff0000u, j0 + 2 * k + 1);
                }
            }
        }
        done = nvec * EPV;
    }
    for (int j = done + lane; j < C; j += 64) ln.push(__float_as_uint(to_f(row[j])), j);
}

template <int KC>
__global__ __launch_bounds__(64 * PD_WAVES) void predict_kernel(const lnx_predict_args a) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * PD_WAVES + (threadIdx.x >> 6);
    if (b >= a.B) return;  // (wave-uniform; the kernel has no barrier)
    const int T = a.n_tasks, K = a.K;
    int kb = K;
    if (a.k_per_sample) {
        kb = a.k_per_sample[b];
        kb = kb < 1 ? 1 : (kb > K ? K : kb);
    }
    int above = -1;       // the consistent node of the task above
    int above_null = -1;  // that task's null class
    for (int t = T - 1; t >= 0; --t) {
        const lnx_predict_task& k = a.task[t];
        Lane<KC> ln;
        ln.init();
        if (a.dtype == 1) scan_row<KC>(ln, static_cast<const bf16_t*>(k.logits) + (int64_t)b * k.ld, k.C, lane);
        else scan_row<KC>(ln, static_cast<const float*>(k.logits) + (int64_t)b * k.ld, k.C, lane);

        // max / sum of the 64 lanes: the pair of the lower lane is always the first operand
        float m = ln.m, s = ln.s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float mo = __shfl_xor(m, o, 64), so = __shfl_xor(s, o, 64);
            const bool upper = (lane & o) != 0;
            const float m0 = upper ? mo : m, s0 = upper ? so : s, m1 = upper ? m : mo, s1 = upper ? s : so;
            const float mm = fmaxf(m0, m1);
            const float e0 = m0 == mm ? 1.0f : expf(m0 - mm), e1 = m1 == mm ? 1.0f : expf(m1 - mm);
            m = mm;
            s = s0 * e0 + s1 * e1;
        }

        // the n best of the row: round r leaves the r-th in lane r
        const int n = kb < k.C ? kb : k.C;
        uint64_t mine = 0, top = 0;
        for (int r = 0; r < n; ++r) {  // (n <= K <= KC, uniform)
            uint64_t w = ln.best[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t other = __shfl_xor(w, o, 64);
                w = other > w ? other : w;
            }
            if (ln.best[0] == w) ln.pop();  // indices are unique: one owner
            if (lane == r) mine = w;
            if (r == 0) top = w;
        }
        const int c = (int)(0xffffffffu - (uint32_t)top);  // the raw top-1 class
        const bool row_nan = (uint32_t)(top >> 32) == 0xffffffffu;

        int flag = 0;
        if (a.consistency && t < T - 1) {
            if (above == above_null && above_null >= 0) flag = 1;
            else if (k.parent[c] != above) flag = 2;
        }
        const bool nullified = flag != 0 && k.null_index >= 0;
        above = nullified ? k.null_index : c;
        above_null = k.null_index;

        const int64_t o = ((int64_t)b * T + t) * K;
        if (lane < K) {
            int cls = -1;
            float p = 0.0f;
            if (nullified) {
                if (lane == 0) {
                    cls = k.null_index;
                    p = 1.0f;
                }
            } else if (lane < n) {
                cls = (int)(0xffffffffu - (uint32_t)mine);
                p = row_nan ? __uint_as_float(0x7fc00000u) : expf(key_value((uint32_t)(mine >> 32)) - m) / s;
            }
            a.ids[o + lane] = cls < 0 ? (int64_t)-1 : (k.id_map ? k.id_map[cls] : (int64_t)cls);
            a.probs[o + lane] = p;
        }
        if (lane == 0) {
            a.count[(int64_t)b * T + t] = nullified ? 1 : n;
            a.flags[(int64_t)b * T + t] = flag;
        }
    }
}

}  // namespace

extern "C" int lnx_predict(const lnx_predict_args* a, void* stream) {
    LNX_CHECK(a, "lnx_predict: NULL arguments");
    LNX_CHECK(a->dtype == 0 || a->dtype == 1, "lnx_predict: dtype=%d (0 = fp32, 1 = bf16)", a->dtype);
    LNX_CHECK(a->K >= 1 && a->K <= LNX_PREDICT_MAX_K, "lnx_predict: K=%d (1..%d)", a->K, LNX_PREDICT_MAX_K);
    LNX_CHECK(a->n_tasks >= 1 && a->n_tasks <= LNX_SOFTCE_MAX_TASKS, "lnx_predict: n_tasks=%d (1..%d)", a->n_tasks, LNX_SOFTCE_MAX_TASKS);
    LNX_CHECK(a->B >= 0, "lnx_predict: B=%d", a->B);
    for (int t = 0; t < a->n_tasks; ++t) {
        const lnx_predict_task& k = a->task[t];
        LNX_CHECK(k.C >= 1, "lnx_predict: task %d has C=%d classes", t, k.C);
        LNX_CHECK(k.ld >= k.C, "lnx_predict: task %d has ld=%lld < C=%d", t, (long long)k.ld, k.C);
        LNX_CHECK(k.logits, "lnx_predict: task %d has NULL logits", t);
        LNX_CHECK(k.null_index < k.C, "lnx_predict: task %d has null_index=%d, C=%d", t, k.null_index, k.C);
        LNX_CHECK(!a->consistency || t == a->n_tasks - 1 || k.parent, "lnx_predict: consistency needs a parent table for task %d (NULL only for the coarsest)", t);
    }
    LNX_CHECK(a->ids && a->probs && a->count && a->flags, "lnx_predict: NULL output (ids / probs / count / flags)");
    if (a->B == 0) return 0;
    const dim3 grid(cdiv(a->B, PD_WAVES)), block(64 * PD_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (a->K <= 4) hipLaunchKernelGGL(predict_kernel<4>, grid, block, 0, st, *a);
    else if (a->K <= 8) hipLaunchKernelGGL(predict_kernel<8>, grid, block, 0, st, *a);
    else hipLaunchKernelGGL(predict_kernel<16>, grid, block, 0, st, *a);
    LNX_LAUNCH_CHECK();
    return 0;
}
