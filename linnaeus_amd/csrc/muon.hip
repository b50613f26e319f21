// Muon (linnaeus/optimizers/muon.py:27-65, 126-190) for gfx950: the whole step of every matrix parameter in
// 3 * max(ns_steps) + 3 launches ("Muon's Newton-Schulz ... MFMA work").
//   muon_momentum_kernel   g *= clip coefficient (when given); buf = lerp(buf, g, 1 - mu); u = nesterov ? lerp(g, buf, mu) : buf; X = bf16(u) (transposed when tall);
//                          one sum-of-squares partial per workgroup
//   muon_normalise_kernel  per 32 x 32 tile of X: fold the matrix's partials in a fixed order, X = bf16(X / (||X|| + 1e-7)), X^T
//   muon_ns_kernel<0/1/2>  A = X X^T;  B = c A A + b A;  X = B X + a X (and X^T): grouped NT products, one wave per 32 x 32 output tile,
//                          fragments straight from L2 (every operand of a step fits there), fp32 accumulate, one rounding
//   muon_apply_kernel      p = p * decay - step * O
// Sharded over data-parallel ranks (lnx_muon_partition): lnx_muon_orthogonalize runs all but the last launch over the matrices a rank owns and
//   muon_pack_kernel          writes each O as bf16 in logical row-major order into the rank's segment of the buffer the ranks all-gather;
//   muon_apply_packed_kernel  p = p * decay - step * O for ALL matrices out of the gathered buffer (lnx_muon_apply_packed), the same expression
// Operands are zero-padded to tile multiples (lnx_muon_layout), so no kernel has an edge case: a padded row or column of X gives
// zero rows / columns of A and B and stays zero in X' = B X + a X.  No atomics: the same inputs give the same bits, alone or in a set.
// With a non-finite guard (lnx_step_guard) EVERY launch reads the guard's flag before it touches a tensor and returns when it is set: products over a NaN
// operand would turn the workspace's zero padding, written once and relied on for ever, into NaN.
#include <algorithm>
#include <atomic>
#include <utility>
#include <vector>

#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int T = LNX_MUON_TILE;
constexpr int ELEMS = LNX_MUON_ELEMS;
constexpr float NS_A = 3.4445f, NS_B = -4.7750f, NS_C = 2.0315f;

std::atomic<int64_t> g_launches{0};

// torch.lerp (ATen/native/Lerp.h): the form that is exact at the nearer end
__device__ __forceinline__ float lerp_f(float a, float b, float w) {
    const float d = b - a;
    return fabsf(w) < 0.5f ? a + w * d : b - d * (1.0f - w);
}

// index of the matrix that owns workgroup `block` of an elementwise launch (block_start ascending)
__device__ __forceinline__ int find_mat(const lnx_muon_mat* __restrict__ mats, int n, int block) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mats[mid].block_start <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// element (r, c) of the logical [rows, cols] matrix inside X [mp, np]
__device__ __forceinline__ int64_t x_index(const lnx_muon_mat& d, int r, int c) {
    return d.rows > d.cols ? (int64_t)c * d.np + r : (int64_t)r * d.np + c;
}

// one 4-byte load, uniform across the workgroup; tested behind the table lookups and ahead of the first access to a matrix, a buffer
// or the workspace (as a kernel's first statement it would stand in front of the loads of the other kernel arguments)
__device__ __forceinline__ bool guard_skips(const float* __restrict__ flag) { return flag != nullptr && *flag != 0.f; }

// sumsq / max_norm: the global-norm clip of lnx_adamw_step; every gradient element is scaled as it is read, g itself is not written.
// grad_scale: the loss scale the gradients still carry (lnx_step_guard); total norm = sqrt(sumsq) * inv, the gradient seen (g * inv) * coef
__global__ __launch_bounds__(256) void muon_momentum_kernel(const lnx_muon_mat* __restrict__ mats, int n, char* __restrict__ ws, float* __restrict__ part,
                                                            const float* __restrict__ sumsq, float max_norm, const float* __restrict__ flag,
                                                            const float* __restrict__ grad_scale) {
    __shared__ float red[4];
    const float inv = grad_scale != nullptr ? __fdiv_rn(1.0f, *grad_scale) : 1.0f;
    float coef = 1.0f;
    if (sumsq != nullptr && max_norm > 0.f) coef = fminf(1.0f, max_norm / (sqrtf(*sumsq) * inv + 1e-6f));
    const lnx_muon_mat& d = mats[find_mat(mats, n, blockIdx.x)];
    if (guard_skips(flag)) return;
    float s = 0.f;
    if (d.g != nullptr) {
        bf16_t* __restrict__ X = reinterpret_cast<bf16_t*>(ws + d.x_off);
        const int64_t numel = (int64_t)d.rows * d.cols;
        const int64_t base = (int64_t)(blockIdx.x - d.block_start) * ELEMS;
        const int64_t end = min(numel, base + ELEMS);
        const float mu = d.momentum, omm = d.omm;
        for (int64_t i = base + threadIdx.x; i < end; i += 256) {
            const float g = (d.g[i] * inv) * coef;
            const float b = lerp_f(d.buf[i], g, omm);
            d.buf[i] = b;
            const float u = d.nesterov ? lerp_f(g, b, mu) : b;
            const bf16_t ub = (bf16_t)u;
            const float uf = (float)ub;
            s += uf * uf;
            X[x_index(d, (int)(i / d.cols), (int)(i % d.cols))] = ub;
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One wave per tile of X (the stage-2 table).  Every wave of a matrix folds the matrix's partials in the same order: same norm bits.
__global__ __launch_bounds__(256) void muon_normalise_kernel(const lnx_muon_mat* __restrict__ mats, const lnx_muon_tile* __restrict__ tiles, int ntiles,
                                                             char* __restrict__ ws, const float* __restrict__ part, const float* __restrict__ flag) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= ntiles) return;
    const lnx_muon_tile tl = tiles[t];
    const lnx_muon_mat& d = mats[tl.mat];
    if (d.g == nullptr || guard_skips(flag)) return;
    const int nblk = (int)(((int64_t)d.rows * d.cols + ELEMS - 1) / ELEMS);
    float s = 0.f;
    for (int i = lane; i < nblk; i += 64) s += part[d.block_start + i];
    s = wave_sum(s);
    const float nrm = __fsqrt_rn(s) + 1e-7f;
    bf16_t* __restrict__ X = reinterpret_cast<bf16_t*>(ws + d.x_off);
    bf16_t* __restrict__ XT = reinterpret_cast<bf16_t*>(ws + d.xt_off[0]);
    const int r = tl.tr * T + (lane >> 1), c0 = tl.tc * T + (lane & 1) * 16;
    bf16_t* row = X + (int64_t)r * d.np + c0;
    uint4 v[2] = {ld16(row), ld16(row + 8)};
    bf16_t* e = reinterpret_cast<bf16_t*>(v);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        e[j] = (bf16_t)__fdiv_rn((float)e[j], nrm);
        XT[(int64_t)(c0 + j) * d.mp + r] = e[j];
    }
    st16(row, v[0]);
    st16(row + 8, v[1]);
}

// Grouped NT product, one wave per T x T output tile: out[i][j] = sum_k P[i][k] Q[j][k], P rows at tile row tr, Q rows at tile column tc.
// The MFMA's first operand is Q and its second P, so a lane ends with FOUR CONSECUTIVE j of one row i (col = lane & 15 -> i,
// row = 4 (lane >> 4) + reg -> j): 8-byte stores.  Lane l's fragment is row (l & 15), k = 8 (l >> 4) .. + 7: one 16-byte load.
//   STAGE 0: A = X X^T            P = Q = X  [mp, np], K = np
//   STAGE 1: B = c A A + b A      P = Q = A  [mp, mp], K = mp (A is symmetric: A A = A A^T)
//   STAGE 2: X = B X + a X        P = B [mp, mp], Q = X^T [np, mp] (ping), K = mp; X in place, X^T to pong
template <int STAGE>
__global__ __launch_bounds__(256) void muon_ns_kernel(const lnx_muon_mat* __restrict__ mats, const lnx_muon_tile* __restrict__ tiles, int ntiles, int it,
                                                      char* __restrict__ ws, const float* __restrict__ flag) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= ntiles) return;
    const lnx_muon_tile tl = tiles[t];
    const lnx_muon_mat& d = mats[tl.mat];
    if (d.g == nullptr || it >= d.ns_steps || guard_skips(flag)) return;
    const int mp = d.mp, np = d.np;
    const bf16_t *P, *Q;
    int K, ldp, ldq;
    if (STAGE == 0) {
        P = Q = reinterpret_cast<const bf16_t*>(ws + d.x_off);
        K = ldp = ldq = np;
    } else if (STAGE == 1) {
        P = Q = reinterpret_cast<const bf16_t*>(ws + d.a_off);
        K = ldp = ldq = mp;
    } else {
        P = reinterpret_cast<const bf16_t*>(ws + d.b_off);
        Q = reinterpret_cast<const bf16_t*>(ws + d.xt_off[it & 1]);
        K = ldp = ldq = mp;
    }
    const int s = lane & 15, g = lane >> 4;
    const bf16_t* p0 = P + (int64_t)(tl.tr * T + s) * ldp + 8 * g;
    const bf16_t* q0 = Q + (int64_t)(tl.tc * T + s) * ldq + 8 * g;
    const int64_t p16 = (int64_t)16 * ldp, q16 = (int64_t)16 * ldq;
    f32x4_t acc[2][2] = {};
    auto mma = [&](const uint4& pa, const uint4& pb, const uint4& qa, const uint4& qb) __attribute__((always_inline)) {
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, qa), __builtin_bit_cast(bf16x8_t, pa), acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, qb), __builtin_bit_cast(bf16x8_t, pa), acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, qa), __builtin_bit_cast(bf16x8_t, pb), acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, qb), __builtin_bit_cast(bf16x8_t, pb), acc[1][1], 0, 0, 0);
    };
    // the next step's fragments are in flight while this step's four MFMAs run (K >= 32 always)
    uint4 pa = ld16(p0), pb = ld16(p0 + p16), qa = ld16(q0), qb = ld16(q0 + q16);
    for (int k = 32; k < K; k += 32) {
        const uint4 na = ld16(p0 + k), nb = ld16(p0 + p16 + k), ma = ld16(q0 + k), mb = ld16(q0 + q16 + k);
        mma(pa, pb, qa, qb);
        pa = na, pb = nb, qa = ma, qb = mb;
    }
    mma(pa, pb, qa, qb);
    // epilogue: lane holds out[i][j .. j + 3], i = tr T + 16 mi + s, j = tc T + 16 ni + 4 g
    bf16_t* out;
    int ldo;
    if (STAGE == 0) {
        out = reinterpret_cast<bf16_t*>(ws + d.a_off);
        ldo = mp;
    } else if (STAGE == 1) {
        out = reinterpret_cast<bf16_t*>(ws + d.b_off);
        ldo = mp;
    } else {
        out = reinterpret_cast<bf16_t*>(ws + d.x_off);
        ldo = np;
    }
    const bf16_t* res = STAGE == 1 ? reinterpret_cast<const bf16_t*>(ws + d.a_off) : out;  // STAGE 2: X itself, the lane's own four elements
    bf16_t* XTn = reinterpret_cast<bf16_t*>(ws + d.xt_off[(it + 1) & 1]);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int i = tl.tr * T + 16 * mi + s, j = tl.tc * T + 16 * ni + 4 * g;
            const int64_t o = (int64_t)i * ldo + j;
            float v[4] = {acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]};
            if (STAGE != 0) {
                const uint2 rr = *reinterpret_cast<const uint2*>(res + o);
                const bf16_t* re = reinterpret_cast<const bf16_t*>(&rr);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = STAGE == 1 ? fmaf(NS_C, v[r], NS_B * (float)re[r]) : fmaf(NS_A, (float)re[r], v[r]);
            }
            uint2 w;
            bf16_t* we = reinterpret_cast<bf16_t*>(&w);
#pragma unroll
            for (int r = 0; r < 4; ++r) we[r] = (bf16_t)v[r];
            *reinterpret_cast<uint2*>(out + o) = w;
            if (STAGE == 2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) XTn[(int64_t)(j + r) * mp + i] = we[r];
            }
        }
}

// the update, one expression for both apply kernels: the sharded step gives the bits of the unsharded one
__device__ __forceinline__ float muon_update(float p, float o, float decay, float nstep) { return fmaf(nstep, o, p * decay); }

__global__ __launch_bounds__(256) void muon_apply_kernel(const lnx_muon_mat* __restrict__ mats, int n, const char* __restrict__ ws, const float* __restrict__ flag) {
    const lnx_muon_mat& d = mats[find_mat(mats, n, blockIdx.x)];
    if (d.g == nullptr || guard_skips(flag)) return;
    const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(ws + d.x_off);
    const int64_t numel = (int64_t)d.rows * d.cols;
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * ELEMS;
    const int64_t end = min(numel, base + ELEMS);
    const float decay = d.decay, nstep = -d.step;
    for (int64_t i = base + threadIdx.x; i < end; i += 256) {
        const float o = (float)X[x_index(d, (int)(i / d.cols), (int)(i % d.cols))];
        d.p[i] = muon_update(d.p[i], o, decay, nstep);
    }
}

// The sharded step's hand-over: O of every owned matrix as bf16 in logical [rows, cols] row-major order at seg + out_off[matrix]
// (multiples of 128 elements in a 256-byte aligned segment).  A thread takes four consecutive logical elements: one 8-byte store, and
// one 8-byte load where they are consecutive in X too (a wide matrix whose cols is a multiple of 4); a tall matrix is un-transposed
// by four strided 2-byte loads.  The last numel % 4 elements of a matrix are stored one by one.
__global__ __launch_bounds__(256) void muon_pack_kernel(const lnx_muon_mat* __restrict__ mats, int n, const char* __restrict__ ws,
                                                        const int64_t* __restrict__ out_off, bf16_t* __restrict__ seg, const float* __restrict__ flag) {
    const int m = find_mat(mats, n, blockIdx.x);
    const lnx_muon_mat& d = mats[m];
    if (d.g == nullptr || guard_skips(flag)) return;
    const bf16_t* __restrict__ X = reinterpret_cast<const bf16_t*>(ws + d.x_off);
    bf16_t* __restrict__ out = seg + out_off[m];
    const int64_t numel = (int64_t)d.rows * d.cols;
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * ELEMS;
    const int64_t end = min(numel, base + ELEMS);
    const bool wide4 = d.rows <= d.cols && (d.cols & 3) == 0;
    for (int64_t i = base + 4 * (int64_t)threadIdx.x; i < end; i += 1024) {
        if (i + 4 <= end) {
            uint2 w;
            if (wide4) {
                w = *reinterpret_cast<const uint2*>(X + x_index(d, (int)(i / d.cols), (int)(i % d.cols)));
            } else {
                bf16_t* we = reinterpret_cast<bf16_t*>(&w);
#pragma unroll
                for (int j = 0; j < 4; ++j) we[j] = X[x_index(d, (int)((i + j) / d.cols), (int)((i + j) % d.cols))];
            }
            *reinterpret_cast<uint2*>(out + i) = w;
        } else {
            for (int64_t k = i; k < end; ++k) out[k] = X[x_index(d, (int)(k / d.cols), (int)(k % d.cols))];
        }
    }
}

// index of the entry that owns workgroup `block` (block_start ascending)
__device__ __forceinline__ int find_packed(const lnx_muon_packed* __restrict__ t, int n, int block) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t[mid].block_start <= block) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// p = p * decay - step * O over the gathered buffer: both operands contiguous.  A thread takes four consecutive elements: p as one
// 16-byte load and store, O as one 8-byte load, when the two addresses allow it (uniform over the workgroup); the last numel % 4
// elements, and a misaligned entry, go one by one.
__global__ __launch_bounds__(256) void muon_apply_packed_kernel(const lnx_muon_packed* __restrict__ table, int n, const bf16_t* __restrict__ gathered,
                                                                const float* __restrict__ flag) {
    const lnx_muon_packed& d = table[find_packed(table, n, blockIdx.x)];
    if (d.off < 0 || guard_skips(flag)) return;
    float* __restrict__ p = d.p;
    const bf16_t* __restrict__ o = gathered + d.off;
    const int64_t base = (int64_t)(blockIdx.x - d.block_start) * ELEMS;
    const int64_t end = min(d.numel, base + ELEMS);
    const float decay = d.decay, nstep = -d.step;
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0 && (reinterpret_cast<uintptr_t>(o) & 7) == 0;
    for (int64_t i = base + 4 * (int64_t)threadIdx.x; i < end; i += 1024) {
        if (vec && i + 4 <= end) {
            float4 pv = *reinterpret_cast<const float4*>(p + i);
            const uint2 ow = *reinterpret_cast<const uint2*>(o + i);
            const bf16_t* oe = reinterpret_cast<const bf16_t*>(&ow);
            pv.x = muon_update(pv.x, (float)oe[0], decay, nstep);
            pv.y = muon_update(pv.y, (float)oe[1], decay, nstep);
            pv.z = muon_update(pv.z, (float)oe[2], decay, nstep);
            pv.w = muon_update(pv.w, (float)oe[3], decay, nstep);
            *reinterpret_cast<float4*>(p + i) = pv;
        } else {
            const int64_t stop = min(end, i + 4);
            for (int64_t k = i; k < stop; ++k) p[k] = muon_update(p[k], (float)o[k], decay, nstep);
        }
    }
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// geometry of one list of shapes; tiles may be NULL
int layout(const int* shapes, int n, lnx_muon_mat* mats, lnx_muon_tile* tiles, int64_t tile_cap, lnx_muon_info* info) {
    int64_t off = 0, nt[3] = {0, 0, 0}, blocks = 0;
    for (int i = 0; i < n; ++i) {
        const int rows = shapes[2 * i], cols = shapes[2 * i + 1];
        LNX_CHECK(rows > 0 && cols > 0, "lnx_muon_layout: matrix %d has shape [%d, %d]", i, rows, cols);
        LNX_CHECK(rows <= (1 << 20) && cols <= (1 << 20) && (int64_t)round_up(rows, T) * round_up(cols, T) < ((int64_t)1 << 31),
                  "lnx_muon_layout: matrix %d [%d, %d] is too large (padded size must stay below 2^31 elements)", i, rows, cols);
        lnx_muon_mat& d = mats[i];
        d.rows = rows;
        d.cols = cols;
        d.mp = round_up(rows < cols ? rows : cols, T);
        d.np = round_up(rows < cols ? cols : rows, T);
        const int64_t xb = (int64_t)d.mp * d.np * 2, ab = (int64_t)d.mp * d.mp * 2;  // multiples of 2048 bytes: every region stays 256-byte aligned
        d.x_off = off;
        d.xt_off[0] = off + xb;
        d.xt_off[1] = off + 2 * xb;
        d.a_off = off + 3 * xb;
        d.b_off = off + 3 * xb + ab;
        off += 3 * xb + 2 * ab;
        const int64_t tm = d.mp / T, tn = d.np / T;
        const int64_t cnt[3] = {tm * tm, tm * tm, tm * tn};
        for (int s = 0; s < 3; ++s) {
            d.tile_start[s] = (int)nt[s];
            d.tile_count[s] = (int)cnt[s];
            nt[s] += cnt[s];
        }
        d.block_start = (int)blocks;
        blocks += ((int64_t)rows * cols + ELEMS - 1) / ELEMS;
        LNX_CHECK(nt[2] < ((int64_t)1 << 30) && blocks < ((int64_t)1 << 30), "lnx_muon_layout: too many tiles or workgroups at matrix %d", i);
    }
    info->workspace_bytes = off;
    for (int s = 0; s < 3; ++s) info->ntiles[s] = nt[s];
    info->total_blocks = (int)blocks;
    if (tiles != nullptr) {
        LNX_CHECK(tile_cap >= nt[0] + nt[1] + nt[2], "lnx_muon_layout: the tile tables need %lld entries, %lld given", (long long)(nt[0] + nt[1] + nt[2]),
                  (long long)tile_cap);
        int64_t base = 0;
        for (int s = 0; s < 3; ++s) {
            for (int i = 0; i < n; ++i) {
                const int tm = mats[i].mp / T, tc_n = s == 2 ? mats[i].np / T : tm;
                lnx_muon_tile* out = tiles + base + mats[i].tile_start[s];
                for (int tr = 0; tr < tm; ++tr)
                    for (int tc = 0; tc < tc_n; ++tc) *out++ = lnx_muon_tile{i, tr, tc, 0};
            }
            base += nt[s];
        }
    }
    return 0;
}

}  // namespace

extern "C" int lnx_muon_layout(const int* shapes, int n, lnx_muon_mat* mats, lnx_muon_tile* tiles, int64_t tile_cap, lnx_muon_info* info) {
    LNX_CHECK(shapes && mats && info && n > 0, "lnx_muon_layout: bad arguments (shapes, mats and info must be given, n > 0)");
    return layout(shapes, n, mats, tiles, tile_cap, info);
}

extern "C" int64_t lnx_muon_launches(void) { return g_launches.load(); }

namespace {

// What lnx_muon_step and lnx_muon_orthogonalize share.  check_step: every check of the arguments, nothing launched; launch_front: the
// momentum, normalise and Newton-Schulz launches (2 + 3 * max_steps).
struct StepPlan {
    lnx_muon_info info;
    int max_steps;
    const float* flag;
};

int check_step(const lnx_muon_step_args* a, const char* who, StepPlan* plan) {
    LNX_CHECK(a != nullptr, "%s: args is NULL", who);
    LNX_CHECK(a->n > 0 && a->mats && a->mats_dev && a->tiles_dev && a->workspace && a->partials, "%s: bad arguments (n > 0 and no NULL table, workspace or partials)", who);
    LNX_CHECK((reinterpret_cast<uintptr_t>(a->workspace) & 255) == 0, "%s: the workspace must be 256-byte aligned", who);
    LNX_CHECK(a->guard == nullptr || a->guard->flag != nullptr, "%s: the guard has no flag", who);
    plan->flag = a->guard != nullptr ? a->guard->flag : nullptr;
    const int n = a->n;
    // the host table must be what lnx_muon_layout gives for its shapes: every offset and tile range the kernels follow is checked here
    std::vector<int> shapes(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        shapes[2 * i] = a->mats[i].rows;
        shapes[2 * i + 1] = a->mats[i].cols;
    }
    std::vector<lnx_muon_mat> ref((size_t)n);
    lnx_muon_info& info = plan->info;
    if (int rc = layout(shapes.data(), n, ref.data(), nullptr, 0, &info)) return rc;
    LNX_CHECK(info.workspace_bytes <= a->workspace_bytes, "%s: the layout needs %lld workspace bytes, %lld given", who, (long long)info.workspace_bytes,
              (long long)a->workspace_bytes);
    int max_steps = 0;
    for (int i = 0; i < n; ++i) {
        const lnx_muon_mat &m = a->mats[i], &r = ref[i];
        bool same = m.mp == r.mp && m.np == r.np && m.x_off == r.x_off && m.xt_off[0] == r.xt_off[0] && m.xt_off[1] == r.xt_off[1] && m.a_off == r.a_off &&
                    m.b_off == r.b_off && m.block_start == r.block_start;
        for (int s = 0; s < 3; ++s) same = same && m.tile_start[s] == r.tile_start[s] && m.tile_count[s] == r.tile_count[s];
        LNX_CHECK(same, "%s: the table entry of matrix %d does not match the layout of its shape [%d, %d]", who, i, m.rows, m.cols);
        LNX_CHECK(m.ns_steps >= 0, "%s: ns_steps=%d of matrix %d", who, m.ns_steps, i);
        LNX_CHECK(m.p != nullptr, "%s: matrix %d has no parameter pointer", who, i);
        LNX_CHECK(m.g == nullptr || m.buf != nullptr, "%s: matrix %d has a gradient but no momentum buffer", who, i);
        if (m.ns_steps > max_steps) max_steps = m.ns_steps;
    }
    plan->max_steps = max_steps;
    return 0;
}

void launch_front(const lnx_muon_step_args* a, const StepPlan& plan, hipStream_t st) {
    const int n = a->n;
    const lnx_muon_info& info = plan.info;
    const float* flag = plan.flag;
    char* ws = static_cast<char*>(a->workspace);
    const lnx_muon_tile* tb[3] = {a->tiles_dev, a->tiles_dev + info.ntiles[0], a->tiles_dev + info.ntiles[0] + info.ntiles[1]};
    hipLaunchKernelGGL(muon_momentum_kernel, dim3(info.total_blocks), dim3(256), 0, st, a->mats_dev, n, ws, a->partials, a->sumsq, a->max_norm, flag,
                       a->guard != nullptr ? a->guard->grad_scale : nullptr);
    hipLaunchKernelGGL(muon_normalise_kernel, dim3(cdiv(info.ntiles[2], 4)), dim3(256), 0, st, a->mats_dev, tb[2], (int)info.ntiles[2], ws, (const float*)a->partials, flag);
    g_launches += 2;
    for (int it = 0; it < plan.max_steps; ++it) {
        // the prefix of each table that still holds a matrix with an iteration left (matrices in descending ns_steps: the others drop out)
        int nt[3] = {0, 0, 0};
        for (int i = 0; i < n; ++i)
            if (a->mats[i].ns_steps > it)
                for (int s = 0; s < 3; ++s) nt[s] = a->mats[i].tile_start[s] + a->mats[i].tile_count[s];
        hipLaunchKernelGGL(muon_ns_kernel<0>, dim3(cdiv(nt[0], 4)), dim3(256), 0, st, a->mats_dev, tb[0], nt[0], it, ws, flag);
        hipLaunchKernelGGL(muon_ns_kernel<1>, dim3(cdiv(nt[1], 4)), dim3(256), 0, st, a->mats_dev, tb[1], nt[1], it, ws, flag);
        hipLaunchKernelGGL(muon_ns_kernel<2>, dim3(cdiv(nt[2], 4)), dim3(256), 0, st, a->mats_dev, tb[2], nt[2], it, ws, flag);
        g_launches += 3;
    }
}

// [off, off + len) of every region with off >= 0: pairwise disjoint?  On overlap, *a and *b name the two entries.
bool regions_disjoint(const std::vector<std::pair<int64_t, int64_t>>& regions, const std::vector<int>& ids, int* a, int* b) {
    std::vector<size_t> idx(regions.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return regions[x].first != regions[y].first ? regions[x].first < regions[y].first : x < y; });
    for (size_t k = 1; k < idx.size(); ++k)
        if (regions[idx[k - 1]].first + regions[idx[k - 1]].second > regions[idx[k]].first) {
            *a = ids[idx[k - 1]];
            *b = ids[idx[k]];
            return false;
        }
    return true;
}

}  // namespace

extern "C" int lnx_muon_step(const lnx_muon_step_args* a, void* stream) {
    StepPlan plan;
    if (int rc = check_step(a, "lnx_muon_step", &plan)) return rc;
    hipStream_t st = (hipStream_t)stream;
    launch_front(a, plan, st);
    hipLaunchKernelGGL(muon_apply_kernel, dim3(plan.info.total_blocks), dim3(256), 0, st, a->mats_dev, a->n, (const char*)a->workspace, plan.flag);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_muon_partition(const int* shapes, const int* ns_steps, int n, int world, int* owner, int64_t* elem_off, int64_t* seg_elems, int64_t* rank_cost) {
    LNX_CHECK(shapes && ns_steps && owner && elem_off && seg_elems && rank_cost && n > 0,
              "lnx_muon_partition: bad arguments (shapes, ns_steps, owner, elem_off, seg_elems and rank_cost must be given, n > 0)");
    LNX_CHECK(world >= 1, "lnx_muon_partition: world=%d, at least one rank is needed", world);
    std::vector<lnx_muon_mat> mats((size_t)n);
    lnx_muon_info info;
    if (int rc = layout(shapes, n, mats.data(), nullptr, 0, &info)) return rc;
    std::vector<int64_t> cost((size_t)n);
    for (int i = 0; i < n; ++i) {
        LNX_CHECK(ns_steps[i] >= 0 && ns_steps[i] <= 1024, "lnx_muon_partition: ns_steps=%d of matrix %d", ns_steps[i], i);
        const int64_t mp = mats[i].mp, np = mats[i].np;  // mp np < 2^31 and mp <= np (lnx_muon_layout): the cost stays far below 2^63
        cost[i] = ns_steps[i] > 0 ? (int64_t)ns_steps[i] * (4 * mp * mp * np + 2 * mp * mp * mp) : mp * np;
        LNX_CHECK(cost[i] < ((int64_t)1 << 56), "lnx_muon_partition: matrix %d [%d, %d] is too costly to count", i, shapes[2 * i], shapes[2 * i + 1]);
    }
    std::vector<int> by_cost((size_t)n);
    for (int i = 0; i < n; ++i) by_cost[i] = i;
    std::stable_sort(by_cost.begin(), by_cost.end(), [&](int x, int y) { return cost[x] > cost[y]; });  // stable: equal costs by ascending index
    for (int r = 0; r < world; ++r) rank_cost[r] = 0;
    for (int i : by_cost) {
        int best = 0;
        for (int r = 1; r < world; ++r)
            if (rank_cost[r] < rank_cost[best]) best = r;  // strict: the lowest rank on ties
        owner[i] = best;
        rank_cost[best] += cost[i];
    }
    std::vector<int64_t> fill((size_t)world, 0);
    int64_t largest = 0;
    for (int i = 0; i < n; ++i) {  // table order inside a segment
        int64_t& f = fill[owner[i]];
        elem_off[i] = f;
        f += ((int64_t)shapes[2 * i] * shapes[2 * i + 1] + LNX_MUON_SEG_ALIGN - 1) / LNX_MUON_SEG_ALIGN * LNX_MUON_SEG_ALIGN;
        if (f > largest) largest = f;
    }
    *seg_elems = largest;
    return 0;
}

extern "C" int lnx_muon_orthogonalize(const lnx_muon_step_args* a, const int64_t* out_off_host, const int64_t* out_off_dev, void* seg, int64_t seg_elems,
                                      void* stream) {
    StepPlan plan;
    if (int rc = check_step(a, "lnx_muon_orthogonalize", &plan)) return rc;
    LNX_CHECK(out_off_host != nullptr && out_off_dev != nullptr, "lnx_muon_orthogonalize: the offset table is NULL (host and device copies must be given)");
    LNX_CHECK(seg != nullptr && seg_elems > 0, "lnx_muon_orthogonalize: no segment (seg=%p, seg_elems=%lld)", seg, (long long)seg_elems);
    LNX_CHECK((reinterpret_cast<uintptr_t>(seg) & 255) == 0, "lnx_muon_orthogonalize: the segment must be 256-byte aligned");
    std::vector<std::pair<int64_t, int64_t>> regions;
    std::vector<int> ids;
    for (int i = 0; i < a->n; ++i) {
        const int64_t off = out_off_host[i], numel = (int64_t)a->mats[i].rows * a->mats[i].cols;
        LNX_CHECK(off >= 0 && off <= seg_elems && numel <= seg_elems - off, "lnx_muon_orthogonalize: matrix %d at offset %lld with %lld elements lies outside the segment of %lld",
                  i, (long long)off, (long long)numel, (long long)seg_elems);
        LNX_CHECK(off % LNX_MUON_SEG_ALIGN == 0, "lnx_muon_orthogonalize: offset %lld of matrix %d is not a multiple of %d elements", (long long)off, i, LNX_MUON_SEG_ALIGN);
        regions.emplace_back(off, numel);
        ids.push_back(i);
    }
    int x = 0, y = 0;
    LNX_CHECK(regions_disjoint(regions, ids, &x, &y), "lnx_muon_orthogonalize: the regions of matrices %d and %d overlap", x, y);
    hipStream_t st = (hipStream_t)stream;
    launch_front(a, plan, st);
    hipLaunchKernelGGL(muon_pack_kernel, dim3(plan.info.total_blocks), dim3(256), 0, st, a->mats_dev, a->n, (const char*)a->workspace, out_off_dev,
                       static_cast<bf16_t*>(seg), plan.flag);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_muon_apply_packed(const lnx_muon_packed* t, const lnx_muon_packed* table_dev, int n, const void* gathered, int64_t seg_elems, int world,
                                     const lnx_step_guard* guard, void* stream) {
    LNX_CHECK(t != nullptr && table_dev != nullptr && n > 0, "lnx_muon_apply_packed: the table is NULL or empty (host and device copies must be given, n > 0)");
    LNX_CHECK(world >= 1, "lnx_muon_apply_packed: world=%d, at least one rank is needed", world);
    LNX_CHECK(gathered != nullptr && seg_elems > 0 && seg_elems % LNX_MUON_SEG_ALIGN == 0 && seg_elems <= (((int64_t)1 << 56) / world),
              "lnx_muon_apply_packed: no gathered buffer, or seg_elems=%lld is not a positive multiple of %d", (long long)seg_elems, LNX_MUON_SEG_ALIGN);
    LNX_CHECK((reinterpret_cast<uintptr_t>(gathered) & 255) == 0, "lnx_muon_apply_packed: the gathered buffer must be 256-byte aligned");
    LNX_CHECK(guard == nullptr || guard->flag != nullptr, "lnx_muon_apply_packed: the guard has no flag");
    const int64_t total = seg_elems * world;
    std::vector<std::pair<int64_t, int64_t>> regions;
    std::vector<int> ids;
    int64_t blocks = 0;
    for (int i = 0; i < n; ++i) {
        const lnx_muon_packed& d = t[i];
        LNX_CHECK(d.numel > 0, "lnx_muon_apply_packed: entry %d has %lld elements", i, (long long)d.numel);
        LNX_CHECK(d.block_start == blocks, "lnx_muon_apply_packed: block_start=%d of entry %d, %lld workgroups lie in front of it", d.block_start, i, (long long)blocks);
        blocks += (d.numel + ELEMS - 1) / ELEMS;
        LNX_CHECK(blocks < ((int64_t)1 << 30), "lnx_muon_apply_packed: too many workgroups at entry %d", i);
        if (d.off < 0) continue;
        LNX_CHECK(d.p != nullptr, "lnx_muon_apply_packed: entry %d has no parameter pointer", i);
        LNX_CHECK(d.off <= total && d.numel <= total - d.off, "lnx_muon_apply_packed: entry %d at offset %lld with %lld elements lies outside the gathered buffer of %lld",
                  i, (long long)d.off, (long long)d.numel, (long long)total);
        regions.emplace_back(d.off, d.numel);
        ids.push_back(i);
    }
    int x = 0, y = 0;
    LNX_CHECK(regions_disjoint(regions, ids, &x, &y), "lnx_muon_apply_packed: the regions of entries %d and %d overlap", x, y);
    hipLaunchKernelGGL(muon_apply_packed_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, table_dev, n, static_cast<const bf16_t*>(gathered),
                       guard != nullptr ? guard->flag : nullptr);
    g_launches += 1;
    LNX_LAUNCH_CHECK();
    return 0;
}
