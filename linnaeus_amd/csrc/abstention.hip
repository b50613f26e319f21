// The abstention phase on [B, C] logits (include/lnx.h: lnx_abstain_act, lnx_ppo_advantages, lnx_ppo_loss_fwd / lnx_ppo_loss_bwd).
// Reference: rl_train_abstention.py:38-131 (compute_gae_and_returns, ppo_update), 133-207 (evaluate_policy) and
// rl_env/reward_functions.py (SimpleAbstentionReward, EpisodeOutcomeReward).
//   abstain_act_kernel   grid B, 256 threads: one workgroup per sample walks the ranks in decision order.  Per row three passes (row_stats,
//                        row_sample): the max and arg-max in strides; exp sums over 256 CONTIGUOUS chunks and an exclusive scan over the
//                        chunk sums, which fixes the running sum of the inverse CDF; the one thread whose chunk holds the crossing walks it
//                        again.  Thread 0 then forms the outcomes, the reward and the counters (integer atomics only).
//   ppo_adv_kernel       ONE workgroup: the GAE recursion per episode, then mean and population std in double (each thread a fixed stride,
//                        a fixed LDS tree), then the normalisation
//   ppo_rows_kernel      grid (B, R): row_stats again -- the same function, so the same bits as the rollout -- and logp at the stored action
//   ppo_fold_kernel      ONE workgroup: ratio, clipped surrogate, value and entropy terms of every transition, their sums in double in a
//                        fixed order, and the transition's d total / d logp for the backward.  A launch of its own behind the row kernel:
//                        the stream orders the two, no workgroup waits for another
//   ppo_bwd_kernel       grid (B, R): dlogits of the taken decisions, dvalue from the workgroups of rank 0
#include <math.h>

#include <atomic>

#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int AB_T = 256;
constexpr int AB_WAVES = AB_T / 64;

std::atomic<int64_t> g_launches{0};  // lnx_abstain_launches

struct RowShared {
    float red[AB_WAVES];
    float best_v[AB_WAVES];
    int best_i[AB_WAVES];
    float wave_tot[AB_WAVES];
    float total;
    int pick;
};

struct RowStats {
    float mx;         // row maximum
    float log_total;  // log of the running sum at the last class; lse = mx + log_total
    float total;
    float H;
    int greedy;
    float chunk_sum;  // this thread's chunk: sum of exp(z - mx) in class order
    float chunk_off;  // the running sum in front of this thread's chunk
};

__device__ __forceinline__ float ab_block_sum(float v, RowShared& sh) {
    v = wave_sum(v);
    __syncthreads();  // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sh.red[0];
#pragma unroll
    for (int w = 1; w < AB_WAVES; ++w) r += sh.red[w];
    return r;
}

__device__ __forceinline__ int ab_block_min(int v, RowShared& sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh.best_i[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = sh.best_i[0];
#pragma unroll
    for (int w = 1; w < AB_WAVES; ++w) r = min(r, sh.best_i[w]);
    return r;
}

// first and last class of thread tid's contiguous chunk
__device__ __forceinline__ void chunk_of(int C, int tid, int& j0, int& j1) {
    const int ch = (C + AB_T - 1) / AB_T;
    j0 = min(tid * ch, C);
    j1 = min(j0 + ch, C);
}

// max, arg-max (lowest index on a tie), the chunked running sum of exp(z - max), entropy.  Every thread of the workgroup calls it; the
// scalars of the result are the same in all of them.
template <typename T>
__device__ __forceinline__ void row_stats(const T* __restrict__ x, int C, RowShared& sh, RowStats& rs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // ---- pass 1: max and arg-max, in strides
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = tid; c < C; c += AB_T) {
        const float v = to_f(x[c]);
        if (v > bv) {  // ascending c per thread: the first maximum stays
            bv = v;
            bi = c;
        }
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
    __syncthreads();  // the slots may still be read by the previous row
    if (lane == 0) {
        sh.best_v[wave] = bv;
        sh.best_i[wave] = bi;
    }
    __syncthreads();
    bv = sh.best_v[0];
    bi = sh.best_i[0];
#pragma unroll
    for (int w = 1; w < AB_WAVES; ++w)
        if (sh.best_v[w] > bv || (sh.best_v[w] == bv && sh.best_i[w] < bi)) {
            bv = sh.best_v[w];
            bi = sh.best_i[w];
        }
    rs.mx = bv;
    rs.greedy = bi == 0x7fffffff ? 0 : bi;  // (a row without any number above -inf: index 0 keeps every read in range)

    // ---- pass 2: this thread's contiguous chunk, in class order
    int j0, j1;
    chunk_of(C, tid, j0, j1);
    float s = 0.f, sz = 0.f;
    for (int j = j0; j < j1; ++j) {
        const float d = to_f(x[j]) - rs.mx;
        const float e = expf(d);
        s += e;
        if (e > 0.f) sz = fmaf(e, d, sz);  // p = 0 contributes 0 (never 0 * -inf)
    }
    // exclusive scan of the chunk sums: inclusive inside the wave, then the waves' totals in order
    float inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) sh.wave_tot[wave] = inc;
    __syncthreads();
    float woff = 0.f;
    for (int w = 0; w < wave; ++w) woff += sh.wave_tot[w];
    rs.chunk_sum = s;
    rs.chunk_off = woff + (inc - s);
    if (tid == AB_T - 1) sh.total = rs.chunk_off + s;  // the running sum at the last class
    const float szt = ab_block_sum(sz, sh);            // (its barriers publish sh.total too)
    rs.total = sh.total;
    rs.log_total = logf(rs.total);
    rs.H = rs.log_total - szt / rs.total;  // lse - sum p z with both terms shifted by the max
}

// the smallest class whose running sum exceeds u * total; the arg-max if rounding leaves none
template <typename T>
__device__ __forceinline__ int row_sample(const T* __restrict__ x, int C, float u, RowShared& sh, const RowStats& rs) {
    const int tid = threadIdx.x;
    const float thr = u * rs.total;
    int j0, j1;
    chunk_of(C, tid, j0, j1);
    // the running sum does not fall inside a chunk, so the first chunk whose last value exceeds thr holds the crossing
    const bool hit = j1 > j0 && rs.chunk_off + rs.chunk_sum > thr;
    const int owner = ab_block_min(hit ? tid : AB_T, sh);
    if (owner == AB_T) return rs.greedy;
    if (tid == owner) {
        float part = 0.f;
        int a = j1 - 1;
        for (int j = j0; j < j1; ++j) {
            part += expf(to_f(x[j]) - rs.mx);  // the additions of pass 2 again: the same bits
            if (rs.chunk_off + part > thr) {
                a = j;
                break;
            }
        }
        sh.pick = a;
    }
    __syncthreads();
    return sh.pick;
}

__device__ __forceinline__ void count_add(int64_t* p, unsigned long long v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), v); }

template <typename T>
__global__ __launch_bounds__(AB_T) void abstain_act_kernel(const lnx_abstain_act_args a) {
    __shared__ RowShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, R = a.R;
    const bool seq = a.mode == LNX_ABSTAIN_SEQUENTIAL;
    bool stopped = false;
    int L = seq ? R : 1;
    unsigned outcomes = 0;  // 4 bits per rank
    for (int r = 0; r < R; ++r) {
        const lnx_abstain_rank& k = a.rank[r];
        const int64_t o = (int64_t)b * R + r;
        int act = k.abstain_index;
        bool pred_none = true;
        if (stopped) {  // (uniform) not taken: the row is not read
            if (tid == 0) {
                a.actions[o] = act;
                a.logp[o] = 0.f;
                a.entropy[o] = 0.f;
                a.taken[o] = 0;
            }
        } else {
            const T* x = static_cast<const T*>(k.logits) + (int64_t)b * k.ld;
            RowStats rs;
            row_stats(x, k.C, sh, rs);
            act = a.greedy ? rs.greedy : row_sample(x, k.C, a.u[o], sh, rs);
            pred_none = act == k.abstain_index;
            if (tid == 0) {
                a.actions[o] = act;
                a.logp[o] = (to_f(x[act]) - rs.mx) - rs.log_total;
                a.entropy[o] = rs.H;
                a.taken[o] = 1;
            }
            if (seq && pred_none) {
                stopped = true;
                L = r + 1;
            }
        }
        const int64_t tg = k.target[b];
        const bool gt_none = tg == k.null_index;
        const unsigned oc = gt_none ? (pred_none ? LNX_ABSTAIN_CORRECT_ABSTAIN : LNX_ABSTAIN_PREDICTED_AT_NULL)
                                    : (pred_none ? LNX_ABSTAIN_UNNECESSARY_ABSTAIN : ((int64_t)act == tg ? LNX_ABSTAIN_CORRECT : LNX_ABSTAIN_MISCLASSIFIED));
        outcomes |= oc << (4 * r);
    }
    if (tid != 0) return;
    const int counted = a.reward_ranks == LNX_ABSTAIN_RANKS_FIRST ? 1 : R;
    float reward;
    if (a.reward_kind == LNX_ABSTAIN_REWARD_SIMPLE) {
        reward = 0.f;
        for (int r = 0; r < counted; ++r) reward += a.table[(outcomes >> (4 * r)) & 15u];
    } else {
        bool optimal = true;
        for (int r = 0; r < counted; ++r) {
            const unsigned oc = (outcomes >> (4 * r)) & 15u;
            if (oc == LNX_ABSTAIN_CORRECT) continue;
            optimal = oc == LNX_ABSTAIN_CORRECT_ABSTAIN;  // the optimal stopping point; anything else is a deviation
            break;
        }
        reward = a.outcome_reward[optimal ? 0 : 1];
    }
    a.reward[b] = reward;
    a.length[b] = L;
    if (a.counts == nullptr) return;
    for (int r = 0; r < R; ++r) {
        int64_t* c = a.counts + LNX_ABSTAIN_CNT_STRIDE * r;
        const unsigned oc = (outcomes >> (4 * r)) & 15u;
        count_add(c + LNX_ABSTAIN_CNT_TOTAL, 1);
        if (oc == LNX_ABSTAIN_CORRECT_ABSTAIN || oc == LNX_ABSTAIN_UNNECESSARY_ABSTAIN) count_add(c + LNX_ABSTAIN_CNT_ABSTAINED, 1);
        const int which = oc == LNX_ABSTAIN_CORRECT_ABSTAIN       ? LNX_ABSTAIN_CNT_CORRECT_ABSTAIN
                          : oc == LNX_ABSTAIN_UNNECESSARY_ABSTAIN ? LNX_ABSTAIN_CNT_UNNECESSARY_ABSTAIN
                          : oc == LNX_ABSTAIN_PREDICTED_AT_NULL   ? LNX_ABSTAIN_CNT_MISSED_ABSTAIN
                          : oc == LNX_ABSTAIN_CORRECT             ? LNX_ABSTAIN_CNT_CORRECT_CLASSIFY
                                                                  : LNX_ABSTAIN_CNT_MISCLASSIFY;
        count_add(c + which, 1);
    }
    count_add(a.counts + LNX_ABSTAIN_CNT_EPISODES, 1);
    count_add(a.counts + LNX_ABSTAIN_CNT_LENGTH_SUM, (unsigned long long)L);
    // two's complement: adding the bits of a negative number subtracts
    count_add(a.counts + LNX_ABSTAIN_CNT_REWARD_FIX, (unsigned long long)llrintf(reward * (float)(1 << LNX_ABSTAIN_REWARD_FIX_BITS)));
}

// fixed LDS tree over the workgroup; every thread gets the sum
__device__ __forceinline__ double tree_sum(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();  // the previous tree is still being read
    red[tid] = v;
    __syncthreads();
    for (int s = AB_T / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(AB_T) void ppo_adv_kernel(const lnx_ppo_adv_args a) {
    __shared__ double red[AB_T];
    const int tid = threadIdx.x, B = a.B, R = a.R;
    const bool seq = a.mode == LNX_ABSTAIN_SEQUENTIAL;
    const float gl = a.gamma * a.gae_lambda;
    // ---- the recursion, episode by episode (raw advantages into adv)
    double s = 0.0, n = 0.0;
    for (int b = tid; b < B; b += AB_T) {
        const int L = seq ? min(max(a.length[b], 1), R) : 1;
        const float V = a.value[b];
        float last = 0.f;
        for (int t = R - 1; t >= 0; --t) {
            const int64_t o = (int64_t)b * R + t;
            if (t >= L) {
                a.adv[o] = 0.f;
                a.ret[o] = 0.f;
                continue;
            }
            const float delta = t == L - 1 ? a.reward[b] - V : a.gamma * V - V;
            last = t == L - 1 ? delta : delta + gl * last;
            a.adv[o] = last;
            a.ret[o] = last + V;
            s += (double)last;
        }
        n += (double)L;
    }
    const double N = tree_sum(n, red);
    const double mean = tree_sum(s, red) / N;
    double q = 0.0;
    for (int b = tid; b < B; b += AB_T) {
        const int L = seq ? min(max(a.length[b], 1), R) : 1;
        for (int t = 0; t < L; ++t) {
            const double d = (double)a.adv[(int64_t)b * R + t] - mean;  // (this thread's own stores)
            q += d * d;
        }
    }
    const double sd = sqrt(tree_sum(q, red) / N);
    const float mean_f = (float)mean, den = (float)sd + 1e-8f;
    for (int b = tid; b < B; b += AB_T) {
        const int L = seq ? min(max(a.length[b], 1), R) : 1;
        for (int t = 0; t < L; ++t) {
            const int64_t o = (int64_t)b * R + t;
            a.adv[o] = (a.adv[o] - mean_f) / den;
        }
    }
    if (tid == 0) a.n_trans[0] = (int)N;
}

__device__ __forceinline__ float* ppo_ws(const lnx_ppo_loss_args& a, int r, int row) { return a.ws + ((int64_t)r * LNX_PPO_WS_ROWS + row) * a.B; }

template <typename T>
__global__ __launch_bounds__(AB_T) void ppo_rows_kernel(const lnx_ppo_loss_args a) {
    __shared__ RowShared sh;
    const int b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const lnx_abstain_rank& k = a.rank[r];
    const int64_t o = (int64_t)b * a.R + r;
    if (a.mode == LNX_ABSTAIN_SEQUENTIAL && !a.taken[o]) {  // (uniform)
        if (tid == 0) {
            ppo_ws(a, r, LNX_PPO_WS_LSE)[b] = 0.f;
            ppo_ws(a, r, LNX_PPO_WS_H)[b] = 0.f;
            ppo_ws(a, r, LNX_PPO_WS_LOGP)[b] = 0.f;
        }
        return;
    }
    const T* x = static_cast<const T*>(k.logits) + (int64_t)b * k.ld;
    RowStats rs;
    row_stats(x, k.C, sh, rs);
    if (tid != 0) return;
    const int act = min(max(a.actions[o], 0), k.C - 1);  // (an action outside the row reads no memory outside it)
    ppo_ws(a, r, LNX_PPO_WS_LSE)[b] = rs.mx + rs.log_total;
    ppo_ws(a, r, LNX_PPO_WS_H)[b] = rs.H;
    ppo_ws(a, r, LNX_PPO_WS_LOGP)[b] = (to_f(x[act]) - rs.mx) - rs.log_total;
}

__global__ __launch_bounds__(AB_T) void ppo_fold_kernel(const lnx_ppo_loss_args a) {
    __shared__ double red[AB_T];
    const int tid = threadIdx.x, B = a.B, R = a.R;
    const bool seq = a.mode == LNX_ABSTAIN_SEQUENTIAL;
    const float lo_c = 1.0f - a.clip_eps, hi_c = 1.0f + a.clip_eps;
    double s_pol = 0.0, s_val = 0.0, s_ent = 0.0, s_ratio = 0.0, s_clip = 0.0, s_n = 0.0;
    for (int b = tid; b < B; b += AB_T) {
        const float V = a.value[b];
        // multitask: one transition of the summed ranks; sequential: one per taken rank
        // (the differences logp_new - logp_old are summed, not the two sums subtracted: small terms, and exactly 0 on a first epoch)
        float dlp = 0.f, H = 0.f;
        for (int r = 0; r < R; ++r) {
            const int64_t o = (int64_t)b * R + r;
            if (seq && !a.taken[o]) {
                ppo_ws(a, r, LNX_PPO_WS_COEF)[b] = 0.f;
                continue;
            }
            if (seq) dlp = H = 0.f;
            dlp += ppo_ws(a, r, LNX_PPO_WS_LOGP)[b] - a.logp_old[o];
            H += ppo_ws(a, r, LNX_PPO_WS_H)[b];
            if (!seq && r < R - 1) continue;
            const int64_t ot = seq ? o : (int64_t)b * R;
            const float A = a.adv[ot], rt = a.ret[ot];
            const float ratio = expf(dlp);
            const float s1 = ratio * A, s2 = fminf(fmaxf(ratio, lo_c), hi_c) * A;
            const float coef = s1 <= s2 ? -A * ratio : 0.f;  // N * d total / d logp_new
            if (seq) ppo_ws(a, r, LNX_PPO_WS_COEF)[b] = coef;
            else
                for (int q = 0; q < R; ++q) ppo_ws(a, q, LNX_PPO_WS_COEF)[b] = coef;
            s_pol += (double)fminf(s1, s2);
            s_val += (double)((V - rt) * (V - rt));
            s_ent += (double)H;
            s_ratio += (double)ratio;
            s_clip += (ratio < lo_c || ratio > hi_c) ? 1.0 : 0.0;
            s_n += 1.0;
        }
    }
    const double N = tree_sum(s_n, red);
    const double pol = tree_sum(s_pol, red), val = tree_sum(s_val, red), ent = tree_sum(s_ent, red);
    const double rat = tree_sum(s_ratio, red), clip = tree_sum(s_clip, red);
    if (tid != 0) return;
    const float policy = (float)(-pol / N), value = (float)(val / N), entropy = (float)(-ent / N);
    a.out[LNX_PPO_OUT_POLICY] = policy;
    a.out[LNX_PPO_OUT_VALUE] = value;
    a.out[LNX_PPO_OUT_ENTROPY] = entropy;
    a.out[LNX_PPO_OUT_TOTAL] = policy + a.vf_coef * value + a.ent_coef * entropy;
    a.out[LNX_PPO_OUT_N] = (float)N;
    a.out[LNX_PPO_OUT_RATIO_MEAN] = (float)(rat / N);
    a.out[LNX_PPO_OUT_CLIP_FRAC] = (float)(clip / N);
}

template <typename T>
__global__ __launch_bounds__(AB_T) void ppo_bwd_kernel(const lnx_ppo_loss_args a, const float* __restrict__ go) {
    const int b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x, R = a.R;
    const bool seq = a.mode == LNX_ABSTAIN_SEQUENTIAL;
    const float g = go[0] / a.out[LNX_PPO_OUT_N];
    if (r == 0 && tid == 0 && a.dvalue) {
        const float V = a.value[b];
        float s = 0.f;
        for (int t = 0; t < (seq ? R : 1); ++t) {
            const int64_t o = (int64_t)b * R + t;
            if (!seq || a.taken[o]) s += V - a.ret[o];
        }
        a.dvalue[b] = 2.0f * a.vf_coef * g * s;
    }
    const lnx_abstain_rank& k = a.rank[r];
    const int64_t o = (int64_t)b * R + r;
    if (k.dlogits == nullptr || (seq && !a.taken[o])) return;  // (uniform) an untaken rank's row stays as it is
    const T* x = static_cast<const T*>(k.logits) + (int64_t)b * k.ld;
    float* d = k.dlogits + (int64_t)b * k.ldd;
    const float lse = ppo_ws(a, r, LNX_PPO_WS_LSE)[b], H = ppo_ws(a, r, LNX_PPO_WS_H)[b];
    const float cp = g * ppo_ws(a, r, LNX_PPO_WS_COEF)[b], ce = g * a.ent_coef;
    const int act = a.actions[o];
    for (int c = tid; c < k.C; c += AB_T) {
        const float z = to_f(x[c]);
        const float p = expf(z - lse);
        // d logp / dz = [c == act] - p;  dH / dz = -p (z - lse + H), and total holds -ent_coef * mean(H)
        const float dh = p > 0.f ? p * (z - lse + H) : 0.f;
        d[c] = cp * ((c == act ? 1.0f : 0.0f) - p) + ce * dh;
    }
}

int ranks_check(const lnx_abstain_rank* rank, int dtype, int B, int R, int mode, bool act, const char* who) {
    LNX_CHECK(R >= 1 && R <= LNX_SOFTCE_MAX_TASKS, "%s: R=%d (1..%d)", who, R, LNX_SOFTCE_MAX_TASKS);
    LNX_CHECK(B > 0, "%s: B=%d", who, B);
    LNX_CHECK(dtype == LNX_F32 || dtype == LNX_BF16, "%s: dtype=%d (0 = fp32, 1 = bf16)", who, dtype);
    LNX_CHECK(mode == LNX_ABSTAIN_MULTITASK || mode == LNX_ABSTAIN_SEQUENTIAL, "%s: mode=%d (0 = multitask, 1 = sequential)", who, mode);
    for (int r = 0; r < R; ++r) {
        const lnx_abstain_rank& k = rank[r];
        LNX_CHECK(k.C > 0, "%s: rank %d has C=%d", who, r, k.C);
        LNX_CHECK(k.ld >= k.C, "%s: rank %d has ld=%lld < C=%d", who, r, (long long)k.ld, k.C);
        LNX_CHECK(k.logits, "%s: rank %d has NULL logits", who, r);
        if (act) {
            LNX_CHECK(k.target, "%s: rank %d has NULL target", who, r);
            LNX_CHECK(k.abstain_index >= 0 && k.abstain_index < k.C, "%s: rank %d has abstain_index=%d outside [0, %d)", who, r, k.abstain_index, k.C);
            LNX_CHECK(k.null_index >= 0 && k.null_index < k.C, "%s: rank %d has null_index=%d outside [0, %d)", who, r, k.null_index, k.C);
        } else {
            LNX_CHECK(k.dlogits == nullptr || k.ldd >= k.C, "%s: rank %d has ldd=%lld < C=%d", who, r, (long long)k.ldd, k.C);
        }
    }
    return 0;
}

int loss_check(const lnx_ppo_loss_args* a, const char* who) {
    LNX_CHECK(a, "%s: NULL arguments", who);
    if (int rc = ranks_check(a->rank, a->dtype, a->B, a->R, a->mode, false, who)) return rc;
    LNX_CHECK(a->actions && a->taken && a->logp_old && a->adv && a->ret && a->value, "%s: NULL actions / taken / logp_old / adv / ret / value", who);
    LNX_CHECK(a->ws && a->out, "%s: NULL ws / out", who);
    LNX_CHECK(a->clip_eps >= 0.f, "%s: clip_eps=%g < 0", who, (double)a->clip_eps);
    return 0;
}

}  // namespace

extern "C" int lnx_abstain_act(const lnx_abstain_act_args* a, void* stream) {
    const char* who = "lnx_abstain_act";
    LNX_CHECK(a, "%s: NULL arguments", who);
    if (int rc = ranks_check(a->rank, a->dtype, a->B, a->R, a->mode, true, who)) return rc;
    LNX_CHECK(a->reward_kind == LNX_ABSTAIN_REWARD_SIMPLE || a->reward_kind == LNX_ABSTAIN_REWARD_OUTCOME, "%s: reward_kind=%d (0 = simple, 1 = outcome)", who,
              a->reward_kind);
    LNX_CHECK(a->reward_ranks == LNX_ABSTAIN_RANKS_ALL || a->reward_ranks == LNX_ABSTAIN_RANKS_FIRST, "%s: reward_ranks=%d (0 = all, 1 = first)", who,
              a->reward_ranks);
    LNX_CHECK(a->greedy || a->u, "%s: sampling needs u (NULL is for greedy only)", who);
    LNX_CHECK(a->actions && a->logp && a->entropy && a->taken && a->length && a->reward, "%s: NULL actions / logp / entropy / taken / length / reward", who);
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == LNX_BF16) hipLaunchKernelGGL(abstain_act_kernel<bf16_t>, dim3(a->B), dim3(AB_T), 0, st, *a);
    else hipLaunchKernelGGL(abstain_act_kernel<float>, dim3(a->B), dim3(AB_T), 0, st, *a);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_ppo_advantages(const lnx_ppo_adv_args* a, void* stream) {
    const char* who = "lnx_ppo_advantages";
    LNX_CHECK(a, "%s: NULL arguments", who);
    LNX_CHECK(a->R >= 1 && a->R <= LNX_SOFTCE_MAX_TASKS, "%s: R=%d (1..%d)", who, a->R, LNX_SOFTCE_MAX_TASKS);
    LNX_CHECK(a->B > 0, "%s: B=%d", who, a->B);
    LNX_CHECK(a->mode == LNX_ABSTAIN_MULTITASK || a->mode == LNX_ABSTAIN_SEQUENTIAL, "%s: mode=%d (0 = multitask, 1 = sequential)", who, a->mode);
    LNX_CHECK(a->reward && a->value && a->adv && a->ret && a->n_trans, "%s: NULL reward / value / adv / ret / n_trans", who);
    LNX_CHECK(a->mode == LNX_ABSTAIN_MULTITASK || a->length, "%s: the sequential mode needs length", who);
    hipLaunchKernelGGL(ppo_adv_kernel, dim3(1), dim3(AB_T), 0, (hipStream_t)stream, *a);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_ppo_loss_fwd(const lnx_ppo_loss_args* a, void* stream) {
    if (int rc = loss_check(a, "lnx_ppo_loss_fwd")) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == LNX_BF16) hipLaunchKernelGGL(ppo_rows_kernel<bf16_t>, dim3(a->B, a->R), dim3(AB_T), 0, st, *a);
    else hipLaunchKernelGGL(ppo_rows_kernel<float>, dim3(a->B, a->R), dim3(AB_T), 0, st, *a);
    hipLaunchKernelGGL(ppo_fold_kernel, dim3(1), dim3(AB_T), 0, st, *a);
    g_launches += 2;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_ppo_loss_bwd(const lnx_ppo_loss_args* a, const float* go_dev, void* stream) {
    if (int rc = loss_check(a, "lnx_ppo_loss_bwd")) return rc;
    LNX_CHECK(go_dev, "lnx_ppo_loss_bwd: NULL go_dev");
    bool any = a->dvalue != nullptr;
    for (int r = 0; r < a->R; ++r) any = any || a->rank[r].dlogits != nullptr;
    LNX_CHECK(any, "lnx_ppo_loss_bwd: neither dvalue nor any rank's dlogits");
    hipStream_t st = (hipStream_t)stream;
    if (a->dtype == LNX_BF16) hipLaunchKernelGGL(ppo_bwd_kernel<bf16_t>, dim3(a->B, a->R), dim3(AB_T), 0, st, *a, go_dev);
    else hipLaunchKernelGGL(ppo_bwd_kernel<float>, dim3(a->B, a->R), dim3(AB_T), 0, st, *a, go_dev);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t lnx_abstain_launches(void) { return g_launches.load(); }
