// The hierarchical loss of the train step in a fixed number of launches (include/lnx.h: lnx_hier_loss_fwd / lnx_hier_loss_bwd).
// Reference: weighted_hierarchical_loss (loss/hierarchical_loss.py:24-406), apply_null_masking / apply_class_weighting /
// apply_loss_masking (loss/masking.py) and GradientWeighting.forward (loss/gradient_weighting.py:301-358).
//   hier_rows_kernel   grid (B, tasks), 256 threads, one sample row per workgroup: the row arithmetic of softce_row (loss.hip), the
//                      null test, the keep decision, the sample's class weight; leaves LNX_HL_WS_ROWS floats per row in ws
//   hier_fold_kernel   ONE workgroup: per task the [B] sums in double (each thread a fixed stride, a fixed LDS tree: the same input
//                      gives the same bits), the denominators, the weighted losses, the gradient scales and the total.  A launch of
//                      its own behind the row kernel: the stream orders the two, so no workgroup ever waits for or signals another
//   hier_bwd_kernel    grid (B, tasks): dlogits from (lse, sum S, coef) of the forward, the fold's scale and the device scalar `go`
#include "common.hpp"
#include "../../include/lnx.h"
#include "taxonomy.hpp"

namespace {

constexpr int HL_T = 256;

__device__ __forceinline__ float hl_block_reduce(float v, float* red, bool is_max) {
    v = is_max ? wave_max(v) : wave_sum(v);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();  // red may still be read from the previous reduction
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

// m * cw^p the way the composed path multiplies: one factor after the other
__device__ __forceinline__ float mul_pow(float m, float cw, int p) {
    for (int i = 0; i < p; ++i) m *= cw;
    return m;
}

// the soft row (or smoothed one-hot row) entry of column c: `at` at the class, `off` elsewhere
__device__ __forceinline__ float soft_at(const float* srow, int c, int64_t t, float at, float off) { return srow ? srow[c] : (c == t ? at : off); }

// (at, off) of the smoothed one-hot row: torch's eps / C everywhere plus 1 - eps at the class, or with LNX_CE_FORM_OFF_TARGET
// 1 - eps at the class and eps / (C - 1) elsewhere (LabelSmoothingCrossEntropy)
__device__ __forceinline__ void smooth_pair(const lnx_hier_loss_task& k, float& at, float& off) {
    const bool off_target = k.form == LNX_CE_FORM_OFF_TARGET;
    const float on = 1.0f - k.smoothing;
    off = k.smoothing / (float)(off_target ? k.C - 1 : k.C);
    at = off_target ? on : on + off;
}

template <typename T>
__global__ __launch_bounds__(HL_T) void hier_rows_kernel(const lnx_hier_loss_args a) {
    __shared__ float red[4];
    __shared__ float best_v[4];
    __shared__ int best_i[4];
    __shared__ TaxRow trow;
    const lnx_hier_loss_task& k = a.task[blockIdx.y];
    const int b = blockIdx.x, tid = threadIdx.x, Cn = k.C;
    const T* x = static_cast<const T*>(k.logits) + (int64_t)b * k.ld;

    // ---- class, null flag, class weight of the sample
    int64_t t;
    bool null;
    float cw = 1.0f, cwc = 1.0f;
    // LNX_CE_FORM_SOFT_ROW: the sample's own target row is S, and <row, crit_weight> the criterion's class weight
    const bool soft_row = k.form == LNX_CE_FORM_SOFT_ROW;
    const float* st = k.soft_target ? k.soft_target + (int64_t)b * k.ldt : nullptr;
    if (st) {
        float bv = -INFINITY, dot = 0.f, cdot = 0.f;
        int bi = 0x7fffffff;
        for (int c = tid; c < Cn; c += HL_T) {
            const float v = st[c];
            if (v > bv) {  // ascending c per thread: the first maximum stays
                bv = v;
                bi = c;
            }
            if (k.class_weight) dot = fmaf(v, k.class_weight[c], dot);
            if (soft_row && k.crit_weight) cdot = fmaf(v, k.crit_weight[c], cdot);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            best_v[tid >> 6] = bv;
            best_i[tid >> 6] = bi;
        }
        __syncthreads();
        bv = best_v[0];
        bi = best_i[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (best_v[w] > bv || (best_v[w] == bv && best_i[w] < bi)) {
                bv = best_v[w];
                bi = best_i[w];
            }
        t = bi == 0x7fffffff ? 0 : bi;  // (a row of NaN / -inf only: torch returns an index too; 0 keeps every read in range)
        null = st[0] > 0.5f;
        if (k.class_weight) cw = hl_block_reduce(dot, red, false);
        if (soft_row && k.crit_weight) cwc = hl_block_reduce(cdot, red, false);
    } else {
        t = k.target[b];
        null = t == 0;
        if (k.class_weight) {
            const int64_t idx = t < 0 ? 0 : (t > k.n_cw - 1 ? k.n_cw - 1 : t);
            cw = t < k.n_cw ? k.class_weight[idx] : 1.0f;
        }
    }

    // ---- the criterion (softce_row)
    bool bad = t < 0 || t >= Cn;
    const bool ignored = k.ignore_index >= 0 && t == k.ignore_index && !soft_row;
    const float* srow = (k.soft != nullptr && !bad && !soft_row) ? k.soft + t * (int64_t)Cn : nullptr;
    // LNX_CE_FORM_TAXONOMY: row t of the matrix is formed per column from the tables (uniform over the workgroup)
    const bool tax = k.form == LNX_CE_FORM_TAXONOMY && !bad;
    if (tax) tax_load(&trow, k.tax_anc, k.tax_val, k.tax_depth, Cn, t);
    float at, off;
    smooth_pair(k, at, off);
    float mx = -INFINITY;
    for (int c = tid; c < Cn; c += HL_T) mx = fmaxf(mx, to_f(x[c]));
    mx = hl_block_reduce(mx, red, true);
    float se = 0.f, sx = 0.f, ss = 0.f;  // sum exp, sum S*x, sum S
    for (int c = tid; c < Cn; c += HL_T) {
        const float v = to_f(x[c]);
        se += __expf(v - mx);
        const float sv = soft_row ? st[c] : (tax ? tax_at(&trow, k.tax_anc, k.tax_depth, Cn, c, t) : soft_at(srow, c, t, at, off));
        sx = fmaf(sv, v, sx);
        ss += sv;
    }
    se = hl_block_reduce(se, red, false);
    sx = hl_block_reduce(sx, red, false);
    ss = hl_block_reduce(ss, red, false);
    if (tid != 0) return;
    const float lse = mx + __logf(se);
    if (soft_row) bad = !(fabsf(ss) < INFINITY);  // NaN or infinite entries in the row: NaN loss, zero gradient row
    else cwc = (k.crit_weight != nullptr && !bad) ? k.crit_weight[t] : 1.0f;
    const float raw = bad ? NAN : (ignored ? 0.f : cwc * (lse * ss - sx));
    const float gcrit = (ignored || bad) ? 0.f : cwc;

    // ---- masking and class weighting
    const bool keep = a.prob >= 1.0f || !null || (a.prob > 0.0f && a.draws[(int64_t)blockIdx.y * a.B + b] < a.prob);
    const float masked = a.mask_mul ? raw * (keep ? 1.0f : 0.0f) : (keep ? raw : 0.0f);
    const float m_cw = mul_pow(masked, cw, k.p_cw);
    const float m_w = mul_pow(m_cw, cw, k.p_w - k.p_cw);
    const float coef = (keep && !(soft_row && bad)) ? mul_pow(gcrit, cw, k.p_w) : 0.0f;  // (a row that is not finite has no finite cw either)
    const unsigned flags = (null ? 1u : 0u) | (keep ? 2u : 0u) | (masked != 0.0f ? 4u : 0u) | (bad ? 0u : (unsigned)t << 3);  // the class for the backward
    float* w = a.ws + (int64_t)blockIdx.y * LNX_HL_WS_ROWS * a.B + b;
    w[(int64_t)LNX_HL_WS_RAW * a.B] = raw;
    w[(int64_t)LNX_HL_WS_LSE * a.B] = lse;
    w[(int64_t)LNX_HL_WS_SS * a.B] = ss;
    w[(int64_t)LNX_HL_WS_COEF * a.B] = coef;
    w[(int64_t)LNX_HL_WS_MASKED_CW * a.B] = m_cw;
    w[(int64_t)LNX_HL_WS_MASKED_W * a.B] = m_w;
    w[(int64_t)LNX_HL_WS_FLAGS * a.B] = __uint_as_float(flags);
}

// six sums of one task over the B rows: raw, masked cw^p_cw, masked cw^p_w in double; null, null & keep, masked != 0 as integers
__global__ __launch_bounds__(HL_T) void hier_fold_kernel(const lnx_hier_loss_args a) {
    __shared__ double fred[3][HL_T];
    __shared__ int ired[3][HL_T];
    const int tid = threadIdx.x, B = a.B;
    float total = 0.f;
    long long null_tot = 0, null_inc = 0;
    for (int t = 0; t < a.n_tasks; ++t) {
        const float* w = a.ws + (int64_t)t * LNX_HL_WS_ROWS * B;
        double f0 = 0.0, f1 = 0.0, f2 = 0.0;
        int i0 = 0, i1 = 0, i2 = 0;
        for (int b = tid; b < B; b += HL_T) {
            f0 += (double)w[(int64_t)LNX_HL_WS_RAW * B + b];
            f1 += (double)w[(int64_t)LNX_HL_WS_MASKED_CW * B + b];
            f2 += (double)w[(int64_t)LNX_HL_WS_MASKED_W * B + b];
            const unsigned fl = __float_as_uint(w[(int64_t)LNX_HL_WS_FLAGS * B + b]);
            i0 += fl & 1u;
            i1 += (fl & 3u) == 3u ? 1 : 0;
            i2 += (fl >> 2) & 1u;
        }
        __syncthreads();  // the previous task's tree is still being read by thread 0
        fred[0][tid] = f0, fred[1][tid] = f1, fred[2][tid] = f2;
        ired[0][tid] = i0, ired[1][tid] = i1, ired[2][tid] = i2;
        __syncthreads();
        for (int s = HL_T / 2; s > 0; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    fred[q][tid] += fred[q][tid + s];
                    ired[q][tid] += ired[q][tid + s];
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const float nv = a.mask_mul ? (float)B : (float)ired[2][0];
            const float wt = a.weights[t];
            const float den = fmaxf(nv, 1e-6f);
            const float weighted = (float)fred[2][0] / den * wt;
            a.out[LNX_HL_OUT_RAW_MEAN * LNX_SOFTCE_MAX_TASKS + t] = (float)(fred[0][0] / (double)B);
            a.out[LNX_HL_OUT_MASKED_MEAN * LNX_SOFTCE_MAX_TASKS + t] = (float)(fred[1][0] / (double)B);
            a.out[LNX_HL_OUT_WEIGHTED * LNX_SOFTCE_MAX_TASKS + t] = weighted;
            a.out[LNX_HL_OUT_SCALE * LNX_SOFTCE_MAX_TASKS + t] = wt / den;
            a.counts[t] = ired[2][0];
            total += weighted;
            null_tot += ired[0][0];
            null_inc += ired[1][0];
        }
    }
    if (tid == 0) {
        a.out[LNX_HL_OUT_TOTAL] = total;
        a.out[LNX_HL_OUT_INCLUSION] = (float)null_inc * 100.0f / fmaxf((float)null_tot, 1.0f);
        a.counts[LNX_HL_NULL_TOTAL] = null_tot;
        a.counts[LNX_HL_NULL_INCLUDED] = null_inc;
    }
}

template <typename T>
__global__ __launch_bounds__(HL_T) void hier_bwd_kernel(const lnx_hier_loss_args a, const float* __restrict__ go) {
    const lnx_hier_loss_task& k = a.task[blockIdx.y];
    if (k.dlogits == nullptr) return;  // (uniform)
    const int b = blockIdx.x, tid = threadIdx.x, Cn = k.C;
    float* d = k.dlogits + (int64_t)b * k.ldd;
    const float* w = a.ws + (int64_t)blockIdx.y * LNX_HL_WS_ROWS * a.B + b;
    const float coef = w[(int64_t)LNX_HL_WS_COEF * a.B];
    if (coef == 0.0f) {  // masked, ignored or out-of-range rows: zeros, whatever the logits hold
        for (int c = tid; c < Cn; c += HL_T) d[c] = 0.0f;
        return;
    }
    const float lse = w[(int64_t)LNX_HL_WS_LSE * a.B], ss = w[(int64_t)LNX_HL_WS_SS * a.B];
    const float g = go[0] * a.out[LNX_HL_OUT_SCALE * LNX_SOFTCE_MAX_TASKS + blockIdx.y] * coef;
    const T* x = static_cast<const T*>(k.logits) + (int64_t)b * k.ld;
    const int64_t t = __float_as_uint(w[(int64_t)LNX_HL_WS_FLAGS * a.B]) >> 3;  // the forward's class (coef != 0: it was in range)
    if (k.form == LNX_CE_FORM_SOFT_ROW) {  // S is the sample's target row, read again
        const float* st = k.soft_target + (int64_t)b * k.ldt;
        for (int c = tid; c < Cn; c += HL_T) {
            const float p = __expf(to_f(x[c]) - lse);
            d[c] = g * (p * ss - st[c]);
        }
        return;
    }
    if (k.form == LNX_CE_FORM_TAXONOMY) {  // S from the tables, as the forward formed it
        __shared__ TaxRow trow;
        tax_load(&trow, k.tax_anc, k.tax_val, k.tax_depth, Cn, t);
        for (int c = tid; c < Cn; c += HL_T) {
            const float p = __expf(to_f(x[c]) - lse);
            d[c] = g * (p * ss - tax_at(&trow, k.tax_anc, k.tax_depth, Cn, c, t));
        }
        return;
    }
    const float* srow = k.soft ? k.soft + t * (int64_t)Cn : nullptr;
    float at, off;
    smooth_pair(k, at, off);
    for (int c = tid; c < Cn; c += HL_T) {
        const float p = __expf(to_f(x[c]) - lse);
        d[c] = g * (p * ss - soft_at(srow, c, t, at, off));
    }
}

int hier_check(const lnx_hier_loss_args* a, const char* who) {
    LNX_CHECK(a, "%s: NULL arguments", who);
    LNX_CHECK(a->n_tasks >= 1 && a->n_tasks <= LNX_SOFTCE_MAX_TASKS, "%s: n_tasks=%d (1..%d)", who, a->n_tasks, LNX_SOFTCE_MAX_TASKS);
    LNX_CHECK(a->B > 0, "%s: B=%d", who, a->B);
    LNX_CHECK(a->dtype == LNX_F32 || a->dtype == LNX_BF16, "%s: dtype=%d (0 = fp32, 1 = bf16)", who, a->dtype);
    LNX_CHECK(a->ws && a->out && a->counts, "%s: NULL ws / out / counts", who);
    LNX_CHECK(a->weights, "%s: NULL weights", who);
    LNX_CHECK(a->prob >= 1.0f || a->prob <= 0.0f || a->draws, "%s: prob=%g < 1 needs draws", who, (double)a->prob);
    for (int t = 0; t < a->n_tasks; ++t) {
        const lnx_hier_loss_task& k = a->task[t];
        LNX_CHECK(k.C > 0 && k.C < (1 << 28), "%s: task %d has C=%d (1 .. 2^28 - 1)", who, t, k.C);
        LNX_CHECK(k.ld >= k.C, "%s: task %d has ld=%lld < C=%d", who, t, (long long)k.ld, k.C);
        LNX_CHECK(k.logits, "%s: task %d has NULL logits", who, t);
        LNX_CHECK((k.target != nullptr) != (k.soft_target != nullptr), "%s: task %d needs exactly one of target / soft_target", who, t);
        LNX_CHECK(k.soft_target == nullptr || k.ldt >= k.C, "%s: task %d has ldt=%lld < C=%d", who, t, (long long)k.ldt, k.C);
        LNX_CHECK(k.smoothing >= 0.f && k.smoothing < 1.f, "%s: task %d has smoothing=%g outside [0, 1)", who, t, (double)k.smoothing);
        LNX_CHECK(k.p_cw >= 0 && k.p_cw <= 3 && k.p_w >= 0 && k.p_w <= 3 && k.p_cw <= k.p_w, "%s: task %d has p_cw=%d p_w=%d (0..3, p_cw <= p_w)", who, t,
                  k.p_cw, k.p_w);
        LNX_CHECK(k.class_weight ? k.n_cw >= 1 : k.p_w == 0, "%s: task %d has class_weight %s with n_cw=%d p_w=%d", who, t,
                  k.class_weight ? "given" : "NULL", k.n_cw, k.p_w);
        LNX_CHECK(!(k.class_weight && k.soft_target) || k.n_cw >= k.C, "%s: task %d has n_cw=%d < C=%d with soft_target", who, t, k.n_cw, k.C);
        LNX_CHECK(k.dlogits == nullptr || k.ldd >= k.C, "%s: task %d has ldd=%lld < C=%d", who, t, (long long)k.ldd, k.C);
        LNX_CHECK(k.form == LNX_CE_FORM_DEFAULT || k.form == LNX_CE_FORM_OFF_TARGET || k.form == LNX_CE_FORM_SOFT_ROW || k.form == LNX_CE_FORM_TAXONOMY,
                  "%s: task %d has form=%d (0 = default, 1 = off-target smoothing, 2 = soft row, 3 = taxonomy tables)", who, t, k.form);
        if (k.form == LNX_CE_FORM_OFF_TARGET) {
            LNX_CHECK(k.C >= 2, "%s: off-target smoothing needs C >= 2, task %d has C=%d (smoothing / (C - 1))", who, t, k.C);
            LNX_CHECK(k.soft == nullptr, "%s: off-target smoothing excludes a [C, C] soft matrix (task %d)", who, t);
        }
        if (k.form == LNX_CE_FORM_SOFT_ROW) {
            LNX_CHECK(k.soft_target, "%s: the soft-row form needs soft_target (task %d)", who, t);
            LNX_CHECK(k.soft == nullptr, "%s: the soft-row form excludes a [C, C] soft matrix (task %d)", who, t);
            LNX_CHECK(k.ignore_index < 0, "%s: the soft-row form has no ignore_index (task %d has %lld)", who, t, (long long)k.ignore_index);
        }
        if (k.form == LNX_CE_FORM_TAXONOMY) {
            LNX_CHECK(k.soft == nullptr, "%s: form=3 (taxonomy tables) excludes a [C, C] soft matrix (task %d)", who, t);
            LNX_CHECK(k.smoothing == 0.f, "%s: form=3 (taxonomy tables) has no uniform smoothing (task %d has %g)", who, t, (double)k.smoothing);
            LNX_CHECK(k.tax_depth >= 0 && k.tax_depth <= LNX_TAX_MAX_DEPTH, "%s: task %d has tax_depth=%d (0..%d)", who, t, k.tax_depth, LNX_TAX_MAX_DEPTH);
            LNX_CHECK(k.tax_val && (k.tax_anc || k.tax_depth == 0), "%s: form=3 (taxonomy tables) needs tax_val, and tax_anc when tax_depth > 0 (task %d)", who, t);
        } else {
            LNX_CHECK(k.tax_anc == nullptr && k.tax_val == nullptr, "%s: task %d has taxonomy tables with form=%d: they belong to form 3", who, t, k.form);
        }
    }
    return 0;
}

}  // namespace

extern "C" int lnx_hier_loss_fwd(const lnx_hier_loss_args* a, void* stream) {
    if (int rc = hier_check(a, "lnx_hier_loss_fwd")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == LNX_BF16) hipLaunchKernelGGL(hier_rows_kernel<bf16_t>, dim3(a->B, a->n_tasks), dim3(HL_T), 0, st, *a);
    else hipLaunchKernelGGL(hier_rows_kernel<float>, dim3(a->B, a->n_tasks), dim3(HL_T), 0, st, *a);
    hipLaunchKernelGGL(hier_fold_kernel, dim3(1), dim3(HL_T), 0, st, *a);
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_hier_loss_bwd(const lnx_hier_loss_args* a, const float* go_dev, void* stream) {
    if (int rc = hier_check(a, "lnx_hier_loss_bwd")) return rc;
    LNX_CHECK(go_dev, "lnx_hier_loss_bwd: NULL go_dev");
    bool any = false;
    for (int t = 0; t < a->n_tasks; ++t) any = any || a->task[t].dlogits != nullptr;
    LNX_CHECK(any, "lnx_hier_loss_bwd: no task has dlogits");
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == LNX_BF16) hipLaunchKernelGGL(hier_bwd_kernel<bf16_t>, dim3(a->B, a->n_tasks), dim3(HL_T), 0, st, *a, go_dev);
    else hipLaunchKernelGGL(hier_bwd_kernel<float>, dim3(a->B, a->n_tasks), dim3(HL_T), 0, st, *a, go_dev);
    LNX_LAUNCH_CHECK();
    return 0;
}
