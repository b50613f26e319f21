// Soft-label cross entropy (forward + logits gradient in one pass) for gfx950.
// Reference: TaxonomyAwareLabelSmoothingCE.forward (loss/taxonomy_label_smoothing.py:233-405):
//   log_probs = log_softmax(logits); per_sample = -sum_c soft_labels[target, c] * log_probs[c];
//   per_sample = 0 where target == ignore_index; per_sample *= class_weight[target] (optional)
// and, with soft == NULL, F.cross_entropy(logits, target, label_smoothing = eps) per sample.
// One 256-thread workgroup per sample row; everything fp32; exp/log only on the row maximum-shifted values.
#include "common.hpp"
#include "../../include/lnx.h"
#include "taxonomy.hpp"

namespace {

__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
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

__device__ __forceinline__ void softce_row(const lnx_softce_args& a, const int b) {
    __shared__ float red[4];
    __shared__ TaxRow trow;
    const float* x = a.logits + (int64_t)b * a.ld;
    // LNX_CE_FORM_SOFT_ROW: the row S is the sample's own target row (SoftTargetCrossEntropy); target is not read
    const float* st = a.form == LNX_CE_FORM_SOFT_ROW ? a.soft_target + (int64_t)b * a.ldt : nullptr;
    const int64_t t = st ? 0 : a.target[b];
    bool bad = t < 0 || t >= a.C;  // out-of-range targets produce NaN loss and zero gradient (the host checks them when asked to)
    const bool ignored = a.ignore_index >= 0 && t == a.ignore_index && !st;
    const float* srow = (a.soft != nullptr && !bad) ? a.soft + t * (int64_t)a.C : nullptr;
    // LNX_CE_FORM_TAXONOMY: row t of the matrix is formed per column from the tables (uniform over the workgroup, like every test above)
    const bool tax = a.form == LNX_CE_FORM_TAXONOMY && !bad;
    if (tax) tax_load(&trow, a.tax_anc, a.tax_val, a.tax_depth, a.C, t);
    // at the class / elsewhere: torch's uniform smoothing, or LabelSmoothingCrossEntropy's eps / (C - 1) off the target only
    const bool off_target = a.form == LNX_CE_FORM_OFF_TARGET;
    const float on = 1.0f - a.smoothing, off = a.smoothing / (float)(off_target ? a.C - 1 : a.C);
    const float at = off_target ? on : on + off;

    float mx = -INFINITY;
    for (int c = threadIdx.x; c < a.C; c += 256) mx = fmaxf(mx, x[c]);
    mx = block_reduce(mx, red, true);
    float se = 0.f, sx = 0.f, ss = 0.f, sw = 0.f;  // sum exp, sum S*x, sum S, sum S*class_weight (soft rows)
    for (int c = threadIdx.x; c < a.C; c += 256) {
        const float v = x[c];
        se += __expf(v - mx);
        const float sv = st ? st[c] : (srow ? srow[c] : (tax ? tax_at(&trow, a.tax_anc, a.tax_depth, a.C, c, t) : (c == t ? at : off)));
        sx = fmaf(sv, v, sx);
        ss += sv;
        if (st && a.class_weight) sw = fmaf(sv, a.class_weight[c], sw);
    }
    se = block_reduce(se, red, false);
    sx = block_reduce(sx, red, false);
    ss = block_reduce(ss, red, false);
    const float lse = mx + __logf(se);
    float cw;
    if (st) {
        bad = !(fabsf(ss) < INFINITY);  // NaN or infinite entries: NaN loss, zero gradient row
        cw = a.class_weight ? block_reduce(sw, red, false) : 1.0f;
    } else {
        cw = (a.class_weight != nullptr && !bad) ? a.class_weight[t] : 1.0f;
    }
    float loss = bad ? NAN : (ignored ? 0.f : cw * (lse * ss - sx));
    const float g = (ignored || bad) ? 0.f : a.scale * (a.row_scale ? a.row_scale[b] : 1.0f) * cw;
    if (threadIdx.x == 0) {
        if (a.loss) a.loss[b] = loss;
        if (a.loss_sum) {
            const float term = a.scale * (a.row_scale ? a.row_scale[b] : 1.0f) * loss;
            if (a.sum_ws) a.sum_ws[b] = term;  // deterministic mode (the entry points decide): folded in row order by launch_fold
            else atomicAdd(a.loss_sum, term);
        }
    }
    if (a.dlogits) {
        float* d = a.dlogits + (int64_t)b * a.ldd;
        const float inv = 1.0f / se;
        if (st && bad) {  // (the row itself is not finite: g * (p * ss - S) would be NaN)
            for (int c = threadIdx.x; c < a.C; c += 256) d[c] = 0.0f;
            return;
        }
        for (int c = threadIdx.x; c < a.C; c += 256) {
            const float p = __expf(x[c] - mx) * inv;
            const float sv = st ? st[c] : (srow ? srow[c] : (tax ? tax_at(&trow, a.tax_anc, a.tax_depth, a.C, c, t) : (c == t ? at : off)));
            d[c] = g * (p * ss - sv);
        }
    }
}

__global__ __launch_bounds__(256) void softce_kernel(const lnx_softce_args a) { softce_row(a, blockIdx.x); }

// all tasks of a multi-task criterion in one launch: blockIdx.y = task (the arguments travel in the kernel-argument segment)
struct SoftceMulti {
    lnx_softce_args a[LNX_SOFTCE_MAX_TASKS];
};
__global__ __launch_bounds__(256) void softce_multi_kernel(const SoftceMulti m) {
    const lnx_softce_args& a = m.a[blockIdx.y];
    if ((int)blockIdx.x < a.B) softce_row(a, blockIdx.x);
}

// lnx_taxonomy_rows: one workgroup per output row
__global__ __launch_bounds__(256) void taxonomy_rows_kernel(const lnx_taxonomy_rows_args a) {
    __shared__ TaxRow trow;
    const int i = blockIdx.x;
    const int64_t r = a.rows ? a.rows[i] : (int64_t)i;
    float* o = a.out + (int64_t)i * a.ldo;
    if (r < 0 || r >= a.C) {  // (uniform over the workgroup)
        for (int c = threadIdx.x; c < a.C; c += 256) o[c] = NAN;
        return;
    }
    tax_load(&trow, a.anc, a.what == 0 ? a.val : nullptr, a.depth, a.C, r);
    for (int c = threadIdx.x; c < a.C; c += 256) {
        const int k = tax_height(&trow, a.anc, a.depth, a.C, c, r);
        o[c] = a.what == 0 ? trow.val[k] : (k > a.depth ? INFINITY : 2.0f * (float)k);
    }
}

}  // namespace

// the argument checks of both entry points, before any launch
static int softce_check(const lnx_softce_args* a, const char* who, int i) {
    const bool soft_row = a->form == LNX_CE_FORM_SOFT_ROW;
    LNX_CHECK(a->form == LNX_CE_FORM_DEFAULT || a->form == LNX_CE_FORM_OFF_TARGET || soft_row || a->form == LNX_CE_FORM_TAXONOMY,
              "%s: form=%d in set %d (0 = default, 1 = off-target smoothing, 2 = soft row, 3 = taxonomy tables)", who, a->form, i);
    LNX_CHECK(a->logits && (a->target || soft_row), "%s: null operand in set %d", who, i);
    LNX_CHECK(a->B > 0 && a->C > 0 && a->ld >= a->C, "%s: bad shape B=%d C=%d ld=%lld in set %d", who, a->B, a->C, (long long)a->ld, i);
    LNX_CHECK(a->dlogits == nullptr || a->ldd >= a->C, "%s: ldd < C in set %d", who, i);
    LNX_CHECK(a->smoothing >= 0.f && a->smoothing < 1.f, "%s: smoothing must be in [0, 1)", who);
    if (a->form == LNX_CE_FORM_OFF_TARGET) {
        LNX_CHECK(a->C >= 2, "%s: off-target smoothing needs C >= 2, set %d has C=%d (smoothing / (C - 1))", who, i, a->C);
        LNX_CHECK(a->soft == nullptr, "%s: off-target smoothing excludes a [C, C] soft matrix (set %d)", who, i);
    }
    if (soft_row) {
        LNX_CHECK(a->soft_target, "%s: the soft-row form needs soft_target (set %d)", who, i);
        LNX_CHECK(a->ldt >= a->C, "%s: ldt=%lld < C=%d in set %d", who, (long long)a->ldt, a->C, i);
        LNX_CHECK(a->soft == nullptr, "%s: the soft-row form excludes a [C, C] soft matrix (set %d)", who, i);
        LNX_CHECK(a->ignore_index < 0, "%s: the soft-row form has no ignore_index (set %d has %lld)", who, i, (long long)a->ignore_index);
    }
    if (a->form == LNX_CE_FORM_TAXONOMY) {
        LNX_CHECK(a->soft == nullptr, "%s: form=3 (taxonomy tables) excludes a [C, C] soft matrix (set %d)", who, i);
        LNX_CHECK(a->smoothing == 0.f, "%s: form=3 (taxonomy tables) has no uniform smoothing (set %d has %g)", who, i, (double)a->smoothing);
        LNX_CHECK(a->tax_depth >= 0 && a->tax_depth <= LNX_TAX_MAX_DEPTH, "%s: tax_depth=%d in set %d (0..%d)", who, a->tax_depth, i, LNX_TAX_MAX_DEPTH);
        LNX_CHECK(a->tax_val && (a->tax_anc || a->tax_depth == 0), "%s: form=3 (taxonomy tables) needs tax_val, and tax_anc when tax_depth > 0 (set %d)", who, i);
    } else {
        LNX_CHECK(a->tax_anc == nullptr && a->tax_val == nullptr, "%s: taxonomy tables given with form=%d (set %d): they belong to form 3", who, a->form, i);
    }
    // the row sums meet in one float atomic per row unless the rows' terms go through sum_ws (deterministic mode)
    LNX_CHECK(a->loss_sum == nullptr || a->sum_ws != nullptr || !deterministic(),
              "%s: deterministic mode needs sum_ws ([B] floats) beside loss_sum in set %d: without it loss_sum is summed by float atomics", who, i);
    return 0;
}

// deterministic mode: loss_sum += the rows' terms in row order; outside it sum_ws is ignored (same kernel path as without it)
static void softce_route(lnx_softce_args& a) {
    if (!deterministic() || a.loss_sum == nullptr) a.sum_ws = nullptr;
}

extern "C" int lnx_softce_multi(const lnx_softce_args* args, int n, void* stream) {
    LNX_CHECK(args && n > 0 && n <= LNX_SOFTCE_MAX_TASKS, "lnx_softce_multi: 1..%d argument sets, got %d", LNX_SOFTCE_MAX_TASKS, n);
    SoftceMulti m;
    int bmax = 0;
    for (int i = 0; i < n; ++i) {
        const lnx_softce_args* a = args + i;
        if (int rc = softce_check(a, "lnx_softce_multi", i)) return rc;
        m.a[i] = *a;
        softce_route(m.a[i]);
        bmax = a->B > bmax ? a->B : bmax;
    }
    hipLaunchKernelGGL(softce_multi_kernel, dim3(bmax, n), dim3(256), 0, (hipStream_t)stream, m);
    for (int i = 0; i < n; ++i)  // (sets may share one loss_sum: set after set)
        if (m.a[i].sum_ws) launch_fold(m.a[i].sum_ws, m.a[i].B, 1, 1, m.a[i].loss_sum, (hipStream_t)stream);
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_softce(const lnx_softce_args* a, void* stream) {
    LNX_CHECK(a, "lnx_softce: null operand");
    if (int rc = softce_check(a, "lnx_softce", 0)) return rc;
    lnx_softce_args q = *a;
    softce_route(q);
    hipLaunchKernelGGL(softce_kernel, dim3(q.B), dim3(256), 0, (hipStream_t)stream, q);
    if (q.sum_ws) launch_fold(q.sum_ws, q.B, 1, 1, q.loss_sum, (hipStream_t)stream);
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_taxonomy_rows(const lnx_taxonomy_rows_args* a, void* stream) {
    LNX_CHECK(a, "lnx_taxonomy_rows: null operand");
    LNX_CHECK(a->C > 0 && a->n > 0, "lnx_taxonomy_rows: bad shape C=%d n=%d", a->C, a->n);
    LNX_CHECK(a->depth >= 0 && a->depth <= LNX_TAX_MAX_DEPTH, "lnx_taxonomy_rows: depth=%d (0..%d)", a->depth, LNX_TAX_MAX_DEPTH);
    LNX_CHECK(a->what == 0 || a->what == 1, "lnx_taxonomy_rows: what=%d (0 = soft labels, 1 = distances)", a->what);
    LNX_CHECK(a->anc || a->depth == 0, "lnx_taxonomy_rows: null anc with depth=%d", a->depth);
    LNX_CHECK(a->val || a->what == 1, "lnx_taxonomy_rows: the soft labels need val");
    LNX_CHECK(a->out && a->ldo >= a->C, "lnx_taxonomy_rows: null out or ldo=%lld < C=%d", (long long)a->ldo, a->C);
    hipLaunchKernelGGL(taxonomy_rows_kernel, dim3(a->n), dim3(256), 0, (hipStream_t)stream, *a);
    LNX_LAUNCH_CHECK();
    return 0;
}
