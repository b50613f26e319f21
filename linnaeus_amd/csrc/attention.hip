// Global multi-head attention with the reference's cos-only "2D RoPE" for gfx950.
//
// Reference: RoPE2DAttention.forward, standard path (blocks/rope_2d_mhsa.py:422-505):
//   q,k image tokens scaled pairwise by cos(theta) (:176-218, finding F1), q *= d^-0.5
//   (:456), S = q k^T in fp32 (:495), softmax (:496), O = P v (:498), O laid out [B,N,h*d].
// Opt-in (rope_mode = LNX_ROPE_ROTATE, template parameter ROT below): the pair rotation by theta that apply_rotary_emb (:176-218)
// computes from the complex table of compute_mixed_cis (:114-155), in the same places as the cos multiply.
// head_dim (HD) is 32, 64 or 128: 64 in every shipped config, and the only one the resident kernels take (the tiled kernels,
// the tables and the freqs fold are templated on it).  N is small (52..580), so the whole problem of a (batch, head) pair is a
// few 64-key tiles; parallelism comes from batch x heads x q-tiles.
//
// Layout trick used everywhere below: score tiles are computed TRANSPOSED (keys in the
// accumulator registers, the query -- or in the dK/dV kernel the key -- on the lane), so
// every per-row softmax quantity is lane-local and the probability tile is already the
// B operand of the next MFMA ("accumulator as operand"); the other operand of that second
// product comes from LDS through ds_read_b64_tr_b16 (bf16) or plain b32 reads (fp32).
//
// Kernels:  attn_fwd  -> o, lse
//           attn_bwd_dq   (per 64 queries: delta, dq, cos-gradient part of q)
//           attn_bwd_dkv  (per 64 keys:    dk, dv, cos-gradient part of k)
//           attn_bwd_res  (resident, N <= 224: both of the above for a whole (sample, head) in one workgroup)
#include <stdlib.h>

#include <atomic>
#include <vector>

#include "common.hpp"
#include "../../include/lnx.h"

namespace {

constexpr int BT = 64;   // rows per tile (queries or keys)

typedef __attribute__((ext_vector_type(4))) short s16x4_t;

template <typename T, int HD = 64> struct AT {
    static_assert(HD == 32 || HD == 64 || HD == 128, "head_dim 32, 64 or 128");
    static constexpr int EPV = TT<T>::EPV;
    static constexpr int NKK = HD * (int)sizeof(T) / 64;  // 64-byte k-chunks per head row (HD 64: 2 bf16 / 4 fp32)
    static constexpr int ND = HD / 16;                    // 16-channel groups of an output row (accumulators per lane)
    static constexpr int ROWB = HD * sizeof(T);           // bytes per row in the row image
    static constexpr int NCH = ROWB / 16;                 // 16-byte chunks per row
    static constexpr int SWZ = (NCH < 8 ? NCH : 8) - 1;   // row-image swizzle mask (r & 7; r & 3 for the 4-chunk bf16 HD 32 row)
    static constexpr int TRB = ROWB + (sizeof(T) == 2 ? 32 : 16);  // padded row bytes of the transposed-read image (HD 64: 160 / 272)
    static constexpr int ROW_IMG = BT * ROWB;
    static constexpr int TR_IMG = BT * TRB;
    // dynamic LDS of the tiled kernels (what each carves out of `smem`; the launchers take the sizes from here)
    static constexpr size_t FWD_LDS = ROW_IMG + TR_IMG;                                      // K~ rows, V transposed (fp32 head_dim 128: 65 KiB)
    static constexpr size_t BWD_DQ_LDS = 2 * ROW_IMG + TR_IMG;                               // K~ rows, V rows, K~ transposed
    static constexpr size_t BWD_DKV_LDS = 2 * ROW_IMG + 2 * TR_IMG + 2 * BT * sizeof(float);  // Q~, dO rows; Q~, dO transposed; lse, delta (fp32 head_dim 128: 130.5 KiB)
};
// dynamic LDS of the resident kernels (bf16 images of a whole sequence padded to npad rows).  The forward pads to whole 64-key tiles
// (npad = qtiles * BT), the backward kernels to 32-row steps (npad = (N + 31) & ~31) plus two statistics per query slot of qtiles tiles.
template <typename T> constexpr size_t res_fwd_lds(int npad) { return (size_t)npad * (AT<T>::ROWB + AT<T>::TRB); }
template <typename T> constexpr size_t res_bwd_dq_lds(int npad) { return (size_t)npad * (2 * AT<T>::TRB); }
template <typename T> constexpr size_t res_bwd_dkv_lds(int npad, int qtiles) { return (size_t)npad * (2 * AT<T>::TRB) + (size_t)qtiles * BT * 2 * sizeof(float); }
// HD^-0.5 as the reference's fp32 product q * head_dim**-0.5 rounds it
template <int HD> constexpr float attn_scale() { return HD == 32 ? 0.17677669529663688f : HD == 64 ? 0.125f : 0.08838834764831845f; }

__device__ __forceinline__ void mfma_bf16(f32x4_t& acc, const uint4& a, const uint4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
}
__device__ __forceinline__ void mfma_f32(f32x4_t& acc, float a, float b) { acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0); }

template <typename T> __device__ __forceinline__ void mfma_chunk(f32x4_t& acc, const uint4& a, const uint4& b) {
    if constexpr (sizeof(T) == 2) {
        mfma_bf16(acc, a, b);
    } else {
        const float* fa = reinterpret_cast<const float*>(&a);
        const float* fb = reinterpret_cast<const float*>(&b);
#pragma unroll
        for (int j = 0; j < 4; ++j) mfma_f32(acc, fa[j], fb[j]);
    }
}

__device__ __forceinline__ uint2 tr_read(const unsigned char* p) {
    const s16x4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
    return __builtin_bit_cast(uint2, v);
}

// One 16-byte chunk (EPV consecutive head channels starting at d0) of token n for the given operand column base,
// optionally multiplied pairwise by cos and by `scale`.  Split in two so that a caller can issue every fetch of a
// batch before the first use: fetch() is unconditional (a row beyond N reads row N - 1, a class token reads the first
// cos row) -- a load under `if (n < N)` whose result is merged with a zero is waited for on the spot, which turns a
// staging loop into one memory round trip per chunk.
// ROT (with COS; LNX_ROPE_ROTATE): the pairs are rotated by theta instead -- the sin table, laid out like the cos table, is fetched
// beside it and value() applies x'[2j] = x[2j] cos - x[2j+1] sin, x'[2j+1] = x[2j] sin + x[2j+1] cos in fp32 before the one rounding.
template <typename T, bool COS, int HD = 64, bool ROT = false> struct Chunk {
    static_assert(COS || !ROT, "a rotated operand is a RoPE operand");
    uint4 raw;
    float cf[COS ? TT<T>::EPV / 2 : 1];
    float sf[ROT ? TT<T>::EPV / 2 : 1];
    __device__ __forceinline__ void fetch(const T* __restrict__ base, int64_t ld, int n, int N, int E, int d0, const float* __restrict__ cos_tab, int heads, int head,
                                          const float* __restrict__ sin_tab = nullptr) {
        const int nc = min(n, N - 1);
        raw = ld16(base + (int64_t)nc * ld + d0);
        if constexpr (COS) {
            const float* cp = cos_tab + ((int64_t)max(nc - E, 0) * heads + head) * (HD / 2) + (d0 >> 1);
            if constexpr (TT<T>::EPV == 8) {
                const float4 c4 = *reinterpret_cast<const float4*>(cp);
                cf[0] = c4.x; cf[1] = c4.y; cf[2] = c4.z; cf[3] = c4.w;
            } else {
                const float2 c2 = *reinterpret_cast<const float2*>(cp);
                cf[0] = c2.x; cf[1] = c2.y;
            }
        }
        if constexpr (ROT) {
            const float* sp = sin_tab + ((int64_t)max(nc - E, 0) * heads + head) * (HD / 2) + (d0 >> 1);
            if constexpr (TT<T>::EPV == 8) {
                const float4 s4 = *reinterpret_cast<const float4*>(sp);
                sf[0] = s4.x; sf[1] = s4.y; sf[2] = s4.z; sf[3] = s4.w;
            } else {
                const float2 s2 = *reinterpret_cast<const float2*>(sp);
                sf[0] = s2.x; sf[1] = s2.y;
            }
        }
    }
    __device__ __forceinline__ uint4 value(int n, int N, int E, float scale) const {
        if (n >= N) return make_uint4(0, 0, 0, 0);
        Vec16<T> v;
        v.raw = raw;
        if constexpr (ROT) {
            constexpr int EPV = TT<T>::EPV;
            if (n >= E) {
#pragma unroll
                for (int j = 0; j < EPV; j += 2) {
                    const float a = v.get(j), b = v.get(j + 1), c = cf[j >> 1], sn = sf[j >> 1];
                    v.set(j, (a * c - b * sn) * scale);
                    v.set(j + 1, (a * sn + b * c) * scale);
                }
            } else if (scale != 1.0f) {
#pragma unroll
                for (int j = 0; j < EPV; ++j) v.set(j, v.get(j) * scale);
            }
        } else if constexpr (COS) {
            constexpr int EPV = TT<T>::EPV;
            if (n >= E) {
#pragma unroll
                for (int j = 0; j < EPV; ++j) v.set(j, v.get(j) * cf[j >> 1] * scale);
            } else if (scale != 1.0f) {
#pragma unroll
                for (int j = 0; j < EPV; ++j) v.set(j, v.get(j) * scale);
            }
        }
        return v.raw;
    }
};

// Staging of a 64-row tile (tokens n0..n0+63) into LDS -- swizzled row image (16-byte fragment reads, rows = MFMA rows) and/or padded
// image for transposed reads -- split in two for the tiled kernels' software pipeline: fetch() requests the tile into registers
// (unconditional, clamped rows -- call it for min(next, last) rather than under `if (more)`), commit() writes it to the LDS
// images one loop trip later, after the products of the current tile have been issued in between.
template <typename T, bool COS, int NT, int HD = 64, bool ROT = false>
struct TileFetch {
    using A = AT<T, HD>;
    static constexpr int NCH = A::NCH, EPV = A::EPV, PER = BT * NCH / NT;
    static_assert(PER > 0 && PER * NT == BT * NCH, "a tile's chunks split evenly over the workgroup");
    Chunk<T, COS, HD, ROT> ch[PER];
    __device__ __forceinline__ void fetch(const T* __restrict__ base, int64_t ld, int n0, int N, int E, const float* __restrict__ cos_tab, int heads, int head,
                                          const float* __restrict__ sin_tab = nullptr) {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = threadIdx.x + u * NT;
            ch[u].fetch(base, ld, n0 + i / NCH, N, E, (i % NCH) * EPV, cos_tab, heads, head, sin_tab);
        }
    }
    template <bool ROWIMG, bool TRIMG>
    __device__ __forceinline__ void commit(unsigned char* rowimg, unsigned char* trimg, int n0, int N, int E, float scale) const {
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = threadIdx.x + u * NT;
            const int r = i / NCH, c = i % NCH;
            const uint4 v = ch[u].value(n0 + r, N, E, scale);
            if constexpr (ROWIMG) st16(rowimg + r * A::ROWB + ((c ^ (r & A::SWZ)) << 4), v);
            if constexpr (TRIMG) st16(trimg + r * A::TRB + c * 16, v);
        }
    }
};

// fragment of a row operand held in registers: lane (s, g) <- token row, chunks kk*4 + g
template <typename T, bool COS, int HD = 64, bool ROT = false>
__device__ __forceinline__ void load_row_frag(uint4 (&f)[(AT<T, HD>::NKK)], const T* __restrict__ base, int64_t ld, int n, int N, int E, int g,
                                              const float* __restrict__ cos_tab, int heads, int head, float scale, const float* __restrict__ sin_tab = nullptr) {
    Chunk<T, COS, HD, ROT> c[(AT<T, HD>::NKK)];
#pragma unroll
    for (int kk = 0; kk < AT<T, HD>::NKK; ++kk) c[kk].fetch(base, ld, n, N, E, (kk * 4 + g) * AT<T, HD>::EPV, cos_tab, heads, head, sin_tab);
#pragma unroll
    for (int kk = 0; kk < AT<T, HD>::NKK; ++kk) f[kk] = c[kk].value(n, N, E, scale);
}

// ---- the two products of every kernel below, with the number NT of live 16-row groups of a tile as a compile-time constant ------
//   rows_times_frag_n      acc[t] (t = 0..3, 16 rows each) = Rows(rowimg, 16 t + s) . frag^T over the HD channels; the groups t >= NT are
//                          padding: skipped, acc = 0
//   rows_times_frag_pad_n  the same product from the PADDED image (rows of TRB = 160 bytes, unswizzled): at that pitch the 16-byte fragment
//                          reads of every 16-lane group of a ds_read_b128 also fall on 16 distinct bank slots, so one image serves both
//                          the row fragments and the transposed reads (half the LDS of keeping a swizzled row image beside it)
//   imgT_times_regs_n      out[dt] += Img^T . P   where P[t][r] holds, for the lane's column, the value of tile row 16 t + 4 g + r
//                          (t = 0..3) -- i.e. contraction over the tile rows; 32-row contraction steps made of padding only are skipped
// With a run-time `nt` every group sits under its own branch: hipcc then emits `ds_read; s_waitcnt lgkmcnt(0); v_mfma` per
// group -- one exposed LDS round trip per pair of MFMAs (round 3: the resident backward kernels spent most of their key /
// query loop that way).  The images are staged in units of 32 rows.  The forward uses NT = 4 for a tile with more than 32 live rows
// (a fourth group of pure padding costs two MFMAs) and NT = 2 for the last tile otherwise; the backward kernels walk in steps of
// NT = 2 throughout (half the live accumulators per step: no scratch).
// PHASE_FENCE keeps the products of one tile step apart: left free, the scheduler hoists the fragment loads of all of them to
// the top and the 128-register budget (two workgroups per CU) spills.
#define PHASE_FENCE() __builtin_amdgcn_sched_barrier(0)
template <int V> struct IC { static constexpr int value = V; };
template <typename T, int NT>
__device__ __forceinline__ void rows_times_frag_pad_n(f32x4_t (&acc)[4], const unsigned char* img, int s, int g, const uint4 (&frag)[AT<T>::NKK]) {
    uint4 a[NT][AT<T>::NKK];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) a[t][kk] = ld16(img + (t * 16 + s) * AT<T>::TRB + ((kk * 4 + g) << 4));
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) mfma_chunk<T>(acc[t], a[t][kk], frag[kk]);
}
template <typename T, int NT, int HD = 64>
__device__ __forceinline__ void rows_times_frag_n(f32x4_t (&acc)[4], const unsigned char* rowimg, int s, int g, const uint4 (&frag)[(AT<T, HD>::NKK)]) {
    using A = AT<T, HD>;
    uint4 a[NT][A::NKK];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < A::NKK; ++kk) a[t][kk] = ld16(rowimg + (t * 16 + s) * A::ROWB + (((kk * 4 + g) ^ ((t * 16 + s) & A::SWZ)) << 4));
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < A::NKK; ++kk) mfma_chunk<T>(acc[t], a[t][kk], frag[kk]);
}
// p[t] of the groups t >= NT must be zero (the image rows behind them may lie beyond the staged part only for t >= 2 ceil(NT / 2))
template <typename T, int NT, int HD = 64>
__device__ __forceinline__ void imgT_times_regs_n(f32x4_t (&out)[HD / 16], const unsigned char* trimg, int s, int g, const float (&p)[4][4]) {
    using A = AT<T, HD>;
    if constexpr (sizeof(T) == 2) {
        constexpr int NKS = (NT + 1) / 2;
        uint4 pf[NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            Vec16<bf16_t> v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v.set(j, p[2 * ks + (j >> 2)][j & 3]);
            pf[ks] = v.raw;
        }
        uint2 a0[NKS][A::ND], a1[NKS][A::ND];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int r0 = ks * 32 + 4 * g + (s >> 2);
#pragma unroll
            for (int dt = 0; dt < A::ND; ++dt) {
                const int col = (dt * 16 + 4 * (s & 3)) * 2;
                a0[ks][dt] = tr_read(trimg + r0 * A::TRB + col);
                a1[ks][dt] = tr_read(trimg + (r0 + 16) * A::TRB + col);
            }
        }
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks)
#pragma unroll
            for (int dt = 0; dt < A::ND; ++dt) mfma_bf16(out[dt], make_uint4(a0[ks][dt].x, a0[ks][dt].y, a1[ks][dt].x, a1[ks][dt].y), pf[ks]);
    } else {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = t * 16 + 4 * g + r;
#pragma unroll
                for (int dt = 0; dt < A::ND; ++dt) {
                    const float a = *reinterpret_cast<const float*>(trimg + row * A::TRB + (dt * 16 + s) * 4);
                    mfma_f32(out[dt], a, p[t][r]);
                }
            }
    }
}

// One HD-element head row held as v[dt][0..3] = elements 16 dt + 4 g .. + 3 by the four lanes g of a row (the layout every
// kernel here ends with).  fp32: HD / 16 16-byte stores.  bf16: lanes g and g ^ 1 swap halves first, so that the even one writes
// elements 16 dt + 4 g .. + 7 of the even dt and the odd one those of the odd dt -- HD / 32 16-byte stores a lane instead of HD / 16
// 8-byte ones (whose half-filled 32-byte sectors made the key-side backward write 1.4x its output).  EVERY lane of the wave must call
// (the exchange is a cross-lane operation); `live` gates the stores only.
template <typename T, int HD = 64> __device__ __forceinline__ void store_row(T* rowp, const float (&v)[HD / 16][4], int g, bool live) {
    constexpr int ND = HD / 16;
    if constexpr (sizeof(T) == 4) {
        if (live) {
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) *reinterpret_cast<float4*>(rowp + dt * 16 + 4 * g) = make_float4(v[dt][0], v[dt][1], v[dt][2], v[dt][3]);
        }
    } else {
        uint2 pk[ND];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            T* h = reinterpret_cast<T*>(&pk[dt]);
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = from_f<T>(v[dt][j]);
        }
        const bool even = (g & 1) == 0;
        if constexpr (ND == 4) {  // head_dim 64: spelled out (the loop form below compiles to a differently scheduled kernel)
            const uint2 s0 = even ? pk[1] : pk[0], s1 = even ? pk[3] : pk[2];
            uint2 r0, r1;
            r0.x = (uint32_t)__shfl_xor((int)s0.x, 16, 64); r0.y = (uint32_t)__shfl_xor((int)s0.y, 16, 64);
            r1.x = (uint32_t)__shfl_xor((int)s1.x, 16, 64); r1.y = (uint32_t)__shfl_xor((int)s1.y, 16, 64);
            if (live) {
                if (even) {
                    st16(rowp + 4 * g, make_uint4(pk[0].x, pk[0].y, r0.x, r0.y));
                    st16(rowp + 32 + 4 * g, make_uint4(pk[2].x, pk[2].y, r1.x, r1.y));
                } else {
                    st16(rowp + 16 + 4 * (g - 1), make_uint4(r0.x, r0.y, pk[1].x, pk[1].y));
                    st16(rowp + 48 + 4 * (g - 1), make_uint4(r1.x, r1.y, pk[3].x, pk[3].y));
                }
            }
        } else {
            uint2 rr[ND / 2];
#pragma unroll
            for (int pp = 0; pp < ND / 2; ++pp) {
                const uint2 sv = even ? pk[2 * pp + 1] : pk[2 * pp];
                rr[pp].x = (uint32_t)__shfl_xor((int)sv.x, 16, 64); rr[pp].y = (uint32_t)__shfl_xor((int)sv.y, 16, 64);
            }
            if (live) {
#pragma unroll
                for (int pp = 0; pp < ND / 2; ++pp) {
                    if (even) st16(rowp + 32 * pp + 4 * g, make_uint4(pk[2 * pp].x, pk[2 * pp].y, rr[pp].x, rr[pp].y));
                    else st16(rowp + 32 * pp + 16 + 4 * (g - 1), make_uint4(rr[pp].x, rr[pp].y, pk[2 * pp + 1].x, pk[2 * pp + 1].y));
                }
            }
        }
    }
}

__device__ __forceinline__ float group_max(float v) {  // over the 4 lanes s, s+16, s+32, s+48
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// sum over the 16 lanes of a DPP row (lanes s = 0..15 of one g): every lane ends with the total
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));  // row_ror:8
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));   // quad_perm [1,0,3,2]
    return v;
}

// Gradient of the learnable RoPE frequencies, reduced where it is produced (round 3; it used to travel through a
// [2][B, N-E, heads, 32] fp32 tensor, ~66 MB per block, written 4 bytes at a time and read back by a separate kernel).
// Autograd of compute_mixed_cis / apply_rotary_emb through the real part only (finding F1):
//   dfreqs[a, h, j] = sum_{b, n} (d cos(theta[n,h,j]) / d freqs[a,h,j]) * gpair[b, n, h, j],   gpair = dQ~[2j] q[2j] + dQ~[2j+1] q[2j+1] (+ the k term)
// This lane holds the 8 pair gradients gp[dt][pr] (j = 8 dt + 2 g + pr) of ONE row and the matching table entries
// dx / dy = -t_x sin(theta), -t_y sin(theta); rows are summed over the 16 lanes of the DPP row, then added to the
// workgroup's HD LDS accumulators [a][j] (order of the LDS float adds is not fixed: last-bit differences from run to run).
// Deterministic mode (fw != NULL): the wave adds to its own slot in global scratch instead -- entry j of a slot belongs to one lane
// (s == 0 of its g), which zeroed it (freq_wave_slot) and is the only one to touch it, in program order; freq_flush folds the slots by
// wave index.
template <int HD = 64>
__device__ __forceinline__ void freq_accum(float* fl, float* fw, const float (&gp)[HD / 16][2], const float (&dx)[HD / 16][2], const float (&dy)[HD / 16][2], int s, int g) {
#pragma unroll
    for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const float tx = row16_sum(gp[dt][pr] * dx[dt][pr]);
            const float ty = row16_sum(gp[dt][pr] * dy[dt][pr]);
            if (s == 0) {
                const int j = 8 * dt + 2 * g + pr;
                if (fw) {
                    fw[j] += tx;
                    fw[HD / 2 + j] += ty;
                } else {
                    atomicAdd(fl + j, tx);
                    atomicAdd(fl + HD / 2 + j, ty);
                }
            }
        }
}
// after the workgroup's last freq_accum: publish (dq kernel) or add to (dk/dv kernel, same grid, launched after it) the partial
constexpr int FREQ_WAVES = 16;  // wave slots per workgroup in the deterministic mode's scratch (the largest backward kernel has 16 waves)
template <bool ADD, int HD = 64> __device__ __forceinline__ void freq_flush(const float* fl, float* fpart, const float* fwave) {
    __syncthreads();
    if (threadIdx.x < HD) {
        float v = fl[threadIdx.x];
        if (fwave) {  // (kernel-uniform)
            const float* b = fwave + (int64_t)blockIdx.x * FREQ_WAVES * HD + threadIdx.x;
            const int nw = blockDim.x >> 6;
            v = 0.f;
            for (int w = 0; w < nw; ++w) v += b[w * HD];
        }
        float* dst = fpart + (int64_t)blockIdx.x * HD + threadIdx.x;
        *dst = ADD ? *dst + v : v;
    }
}

// exp(x - m) with m fixed along a row.  bf16 kernels: log2(e) folded into the subtraction, one FMA in front of v_exp_f32
// (prep(m) = m log2(e) once per row) instead of subtract + multiply; fp32 (strict parity) kernels: libm.  `clamped` bounds the
// argument by 0 -- a no-op for real (query, key) pairs of the backward (x <= lse), it keeps padding entries finite.
template <typename T> struct RowExp {
    static constexpr float L2E = 1.44269504088896340736f;
    static __device__ __forceinline__ float prep(float m) {
        if constexpr (sizeof(T) == 2) return m * L2E;
        else return m;
    }
    static __device__ __forceinline__ float sub(float x, float mp) {
        if constexpr (sizeof(T) == 2) return __builtin_amdgcn_exp2f(fmaf(x, L2E, -mp));
        else return expf(x - mp);
    }
    static __device__ __forceinline__ float clamped(float x, float mp) {
        if constexpr (sizeof(T) == 2) return __builtin_amdgcn_exp2f(fminf(fmaf(x, L2E, -mp), 0.f));
        else return expf(fminf(x - mp, 0.f));
    }
};

struct AttnP {
    const void* qkv;
    const float* cos_tab;
    void* o;
    float* lse;
    const void* d_o;
    void* dqkv;
    float* fpart;        // [workgroups][2][HD/2]: per-workgroup partial sums of the freqs gradient (dq kernel writes, dk/dv kernel adds)
    const float* dsin;   // [2][N-E, heads, HD/2]: -t_x sin(theta), -t_y sin(theta) = d cos(theta) / d freqs[a]
    float* delta;
    int B, N, E, heads;
    int qtiles;
    const unsigned char* amask = nullptr;  // DROP kernels: keep mask [B, heads, N, Np] of the attention probabilities
    float a_inv_keep = 1.0f;
    int Np = 0;                            // N rounded up to a multiple of 64
    const float* sin_tab = nullptr;        // ROT kernels: sin(theta), laid out like cos_tab
    int W = 1;                             // ROT backward: width of the token grid (t_x = n % W, t_y = n / W of image token n)
    float* fwave = nullptr;                // deterministic mode: [workgroups][FREQ_WAVES][HD] per-wave sums of the freqs gradient; else NULL
    const int* nkeep = nullptr;            // compact rows: device int, the problems of samples b >= *nkeep are skipped
};

// this wave's slot of p.fwave, zeroed by the lanes that own its entries (freq_accum); NULL outside the deterministic mode
template <int HD = 64> __device__ __forceinline__ float* freq_wave_slot(const AttnP& p) {
    if (p.fwave == nullptr) return nullptr;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float* fw = p.fwave + ((int64_t)blockIdx.x * FREQ_WAVES + wave) * HD;
    if ((lane & 15) == 0) {
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                const int j = 8 * dt + 2 * (lane >> 4) + pr;
                fw[j] = 0.f;
                fw[HD / 2 + j] = 0.f;
            }
    }
    return fw;
}

// dk / dv epilogue of one 16-key wave tile: every load in one batch (clamped rows, unconditional), 8-/16-byte stores, the k part
// of the freqs gradient.  Shared by the resident and the tiled kernel.
// ROT: dk comes back through the inverse rotation, and the pair gradient is d theta = dk'[2j+1] k'[2j] - dk'[2j] k'[2j+1] (k' = the rotated
// k, recomputed in fp32 from the raw row), weighted by t_x, t_y (from the token index and the grid width) instead of the d-cos table.
template <typename T, int HD = 64, bool ROT = false>
__device__ __forceinline__ void dkv_epilogue(const AttnP& p, const f32x4_t (&dk)[HD / 16], const f32x4_t (&dv)[HD / 16], const T* __restrict__ kb, int64_t ld, int C,
                                             int b, int head, int key, int s, int g, float* fl, float* fw) {
    const int kc = min(key, p.N - 1);
    const T* kraw = kb + (int64_t)kc * ld;
    const float* cpr = p.cos_tab + ((int64_t)max(kc - p.E, 0) * p.heads + head) * (HD / 2);
    const float* sxp = p.dsin + ((int64_t)max(kc - p.E, 0) * p.heads + head) * (HD / 2);
    const float* syp = sxp + (int64_t)(p.N - p.E) * p.heads * (HD / 2);
    constexpr int ND = HD / 16;
    float kr[ND][4], cr[ND][2], gp[ND][2], dx[ND][2], dy[ND][2];
    float sr[ROT ? ND : 1][2];
    const bool rope = p.E < p.N;  // uniform: without image tokens there are no tables
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
        const int d0 = dt * 16 + 4 * g;
        if constexpr (sizeof(T) == 2) {
            const uint2 r = *reinterpret_cast<const uint2*>(kraw + d0);
            const bf16_t* h = reinterpret_cast<const bf16_t*>(&r);
#pragma unroll
            for (int j = 0; j < 4; ++j) kr[dt][j] = (float)h[j];
        } else {
            const float4 r = *reinterpret_cast<const float4*>(kraw + d0);
            kr[dt][0] = r.x; kr[dt][1] = r.y; kr[dt][2] = r.z; kr[dt][3] = r.w;
        }
        cr[dt][0] = cr[dt][1] = 1.0f;
        dx[dt][0] = dx[dt][1] = dy[dt][0] = dy[dt][1] = 0.f;
        if constexpr (ROT) {
            sr[dt][0] = sr[dt][1] = 0.f;
            if (rope) {
                const float2 c2 = *reinterpret_cast<const float2*>(cpr + (d0 >> 1));
                const float2 s2 = *reinterpret_cast<const float2*>(p.sin_tab + ((int64_t)max(kc - p.E, 0) * p.heads + head) * (HD / 2) + (d0 >> 1));
                cr[dt][0] = c2.x; cr[dt][1] = c2.y;
                sr[dt][0] = s2.x; sr[dt][1] = s2.y;
                dx[dt][0] = dx[dt][1] = (float)(max(kc - p.E, 0) % p.W);
                dy[dt][0] = dy[dt][1] = (float)(max(kc - p.E, 0) / p.W);
            }
        } else if (rope) {
            const float2 c2 = *reinterpret_cast<const float2*>(cpr + (d0 >> 1));
            cr[dt][0] = c2.x; cr[dt][1] = c2.y;
            const float2 a2 = *reinterpret_cast<const float2*>(sxp + (d0 >> 1));
            const float2 b2 = *reinterpret_cast<const float2*>(syp + (d0 >> 1));
            dx[dt][0] = a2.x; dx[dt][1] = a2.y;
            dy[dt][0] = b2.x; dy[dt][1] = b2.y;
        }
    }
    const bool row = key < p.N, img = row && key >= p.E;
    T* dkp = reinterpret_cast<T*>(p.dqkv) + ((int64_t)b * p.N + kc) * ld + C + head * HD;
    {
        float ok[ND][4];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            const float c0 = img ? cr[dt][0] : 1.0f, c1 = img ? cr[dt][1] : 1.0f;
            if constexpr (ROT) {
                const float s0 = img ? sr[dt][0] : 0.f, s1 = img ? sr[dt][1] : 0.f;
                ok[dt][0] = dk[dt][0] * c0 + dk[dt][1] * s0; ok[dt][1] = dk[dt][1] * c0 - dk[dt][0] * s0;
                ok[dt][2] = dk[dt][2] * c1 + dk[dt][3] * s1; ok[dt][3] = dk[dt][3] * c1 - dk[dt][2] * s1;
                const float x0 = kr[dt][0] * c0 - kr[dt][1] * s0, x1 = kr[dt][0] * s0 + kr[dt][1] * c0;
                const float x2 = kr[dt][2] * c1 - kr[dt][3] * s1, x3 = kr[dt][2] * s1 + kr[dt][3] * c1;
                gp[dt][0] = img ? dk[dt][1] * x0 - dk[dt][0] * x1 : 0.f;
                gp[dt][1] = img ? dk[dt][3] * x2 - dk[dt][2] * x3 : 0.f;
                continue;
            }
            ok[dt][0] = dk[dt][0] * c0; ok[dt][1] = dk[dt][1] * c0; ok[dt][2] = dk[dt][2] * c1; ok[dt][3] = dk[dt][3] * c1;
            gp[dt][0] = img ? dk[dt][0] * kr[dt][0] + dk[dt][1] * kr[dt][1] : 0.f;
            gp[dt][1] = img ? dk[dt][2] * kr[dt][2] + dk[dt][3] * kr[dt][3] : 0.f;
        }
        store_row<T, HD>(dkp, ok, g, row);
    }
    {
        float ov[ND][4];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[dt][j] = dv[dt][j];
        store_row<T, HD>(dkp + C, ov, g, row);
    }
    if (rope) freq_accum<HD>(fl, fw, gp, dx, dy, s, g);
}
// dq epilogue of one 16-query wave tile (the tiled kernel; the resident one fetches its operands ahead of the key loop)
template <typename T, int HD = 64, bool ROT = false>
__device__ __forceinline__ void dq_epilogue(const AttnP& p, const f32x4_t (&dq)[HD / 16], const T* __restrict__ qb, int64_t ld, int b, int head, int q, int s, int g,
                                            float scale, float* fl, float* fw) {
    const int qc = min(q, p.N - 1);
    const T* qraw = qb + (int64_t)qc * ld;
    const float* cpr = p.cos_tab + ((int64_t)max(qc - p.E, 0) * p.heads + head) * (HD / 2);
    const float* sxp = p.dsin + ((int64_t)max(qc - p.E, 0) * p.heads + head) * (HD / 2);
    const float* syp = sxp + (int64_t)(p.N - p.E) * p.heads * (HD / 2);
    constexpr int ND = HD / 16;
    float qr[ND][4], cr[ND][2], gp[ND][2], dx[ND][2], dy[ND][2];
    float sr[ROT ? ND : 1][2];
    const bool rope = p.E < p.N;
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
        const int d0 = dt * 16 + 4 * g;
        if constexpr (sizeof(T) == 2) {
            const uint2 r = *reinterpret_cast<const uint2*>(qraw + d0);
            const bf16_t* h = reinterpret_cast<const bf16_t*>(&r);
#pragma unroll
            for (int j = 0; j < 4; ++j) qr[dt][j] = (float)h[j];
        } else {
            const float4 r = *reinterpret_cast<const float4*>(qraw + d0);
            qr[dt][0] = r.x; qr[dt][1] = r.y; qr[dt][2] = r.z; qr[dt][3] = r.w;
        }
        cr[dt][0] = cr[dt][1] = 1.0f;
        dx[dt][0] = dx[dt][1] = dy[dt][0] = dy[dt][1] = 0.f;
        if constexpr (ROT) {
            sr[dt][0] = sr[dt][1] = 0.f;
            if (rope) {
                const float2 c2 = *reinterpret_cast<const float2*>(cpr + (d0 >> 1));
                const float2 s2 = *reinterpret_cast<const float2*>(p.sin_tab + ((int64_t)max(qc - p.E, 0) * p.heads + head) * (HD / 2) + (d0 >> 1));
                cr[dt][0] = c2.x; cr[dt][1] = c2.y;
                sr[dt][0] = s2.x; sr[dt][1] = s2.y;
                dx[dt][0] = dx[dt][1] = (float)(max(qc - p.E, 0) % p.W);
                dy[dt][0] = dy[dt][1] = (float)(max(qc - p.E, 0) / p.W);
            }
        } else if (rope) {
            const float2 c2 = *reinterpret_cast<const float2*>(cpr + (d0 >> 1));
            cr[dt][0] = c2.x; cr[dt][1] = c2.y;
            const float2 a2 = *reinterpret_cast<const float2*>(sxp + (d0 >> 1));
            const float2 b2 = *reinterpret_cast<const float2*>(syp + (d0 >> 1));
            dx[dt][0] = a2.x; dx[dt][1] = a2.y;
            dy[dt][0] = b2.x; dy[dt][1] = b2.y;
        }
    }
    const bool row = q < p.N, img = row && q >= p.E;
    T* dqp = reinterpret_cast<T*>(p.dqkv) + ((int64_t)b * p.N + qc) * ld + head * HD;
    float oq[ND][4];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) {
        if constexpr (ROT) {  // dq is the gradient of q~ = scale q': inverse rotation, d theta = dq~[2j+1] q~[2j] - dq~[2j] q~[2j+1]
            const float s0 = img ? sr[dt][0] : 0.f, s1 = img ? sr[dt][1] : 0.f, r0 = img ? cr[dt][0] : 1.0f, r1 = img ? cr[dt][1] : 1.0f;
            oq[dt][0] = scale * (dq[dt][0] * r0 + dq[dt][1] * s0); oq[dt][1] = scale * (dq[dt][1] * r0 - dq[dt][0] * s0);
            oq[dt][2] = scale * (dq[dt][2] * r1 + dq[dt][3] * s1); oq[dt][3] = scale * (dq[dt][3] * r1 - dq[dt][2] * s1);
            const float x0 = qr[dt][0] * r0 - qr[dt][1] * s0, x1 = qr[dt][0] * s0 + qr[dt][1] * r0;
            const float x2 = qr[dt][2] * r1 - qr[dt][3] * s1, x3 = qr[dt][2] * s1 + qr[dt][3] * r1;
            gp[dt][0] = img ? scale * (dq[dt][1] * x0 - dq[dt][0] * x1) : 0.f;
            gp[dt][1] = img ? scale * (dq[dt][3] * x2 - dq[dt][2] * x3) : 0.f;
            continue;
        }
        const float c0 = img ? cr[dt][0] * scale : scale, c1 = img ? cr[dt][1] * scale : scale;
        oq[dt][0] = dq[dt][0] * c0; oq[dt][1] = dq[dt][1] * c0; oq[dt][2] = dq[dt][2] * c1; oq[dt][3] = dq[dt][3] * c1;
        gp[dt][0] = img ? scale * (dq[dt][0] * qr[dt][0] + dq[dt][1] * qr[dt][1]) : 0.f;
        gp[dt][1] = img ? scale * (dq[dt][2] * qr[dt][2] + dq[dt][3] * qr[dt][3]) : 0.f;
    }
    store_row<T, HD>(dqp, oq, g, row);
    if (rope) freq_accum<HD>(fl, fw, gp, dx, dy, s, g);
}

// ---------------------------------------------------------------------------------
// forward: one workgroup = 16 NW queries of one (b, head); wave = 16 queries (lane s).  NW = 8 (bf16, long sequences): every
// staged 64-key tile serves 128 queries, i.e. half the staging work, LDS writes and barriers per query of NW = 4.
// p.qtiles = ceil(N / (16 NW)).
// ---------------------------------------------------------------------------------
// DROP: dropout on the attention probabilities (rope_2d_mhsa.py:497), applied after the normalisation: the running sum
// takes the undropped exponentials, P . V the dropped ones
template <typename T, int NW = 4, bool DROP = false, int HD = 64, bool ROT = false>
__global__ __launch_bounds__(64 * NW) void attn_fwd_kernel(const AttnP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* kimg = smem;                       // K~ row image                 (AT<T, HD>::FWD_LDS bytes in all)
    unsigned char* vimg = smem + AT<T, HD>::ROW_IMG;      // V transposed-read image
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const int qt = blockIdx.x % p.qtiles;
    const int bh = blockIdx.x / p.qtiles;
    const int head = bh % p.heads, b = bh / p.heads;
    if (p.nkeep && b >= *p.nkeep) return;  // compact rows: samples at or beyond the kept count are nobody's (before any staging)
    const int C = p.heads * HD;
    const int64_t ld = 3 * C;
    const T* qb = reinterpret_cast<const T*>(p.qkv) + (int64_t)b * p.N * ld + head * HD;
    const T* kb = qb + C;
    const T* vb = qb + 2 * C;
    const float scale = attn_scale<HD>();  // HD^-0.5

    const int q = qt * (16 * NW) + wave * 16 + s;
    uint4 qf[(AT<T, HD>::NKK)];
    load_row_frag<T, true, HD, ROT>(qf, qb, ld, q, p.N, p.E, g, p.cos_tab, p.heads, head, scale, p.sin_tab);

    f32x4_t oacc[HD / 16];
#pragma unroll
    for (int i = 0; i < HD / 16; ++i) oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const unsigned char* mrow = nullptr;
    if constexpr (DROP) mrow = p.amask + (((int64_t)b * p.heads + head) * p.N + min(q, p.N - 1)) * p.Np + 4 * g;

    const int nkt = (p.N + BT - 1) / BT;
    TileFetch<T, true, 64 * NW, HD, ROT> fk;   // the next key tile travels in registers while this one is multiplied
    TileFetch<T, false, 64 * NW, HD> fv;
    fk.fetch(kb, ld, 0, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
    fv.fetch(vb, ld, 0, p.N, p.E, nullptr, p.heads, head);
    for (int kt = 0; kt < nkt; ++kt) {
        uint32_t mk[4] = {0, 0, 0, 0};
        if constexpr (DROP) {
#pragma unroll
            for (int t = 0; t < 4; ++t) mk[t] = *reinterpret_cast<const uint32_t*>(mrow + kt * BT + 16 * t);
        }
        __syncthreads();
        fk.template commit<true, false>(kimg, nullptr, kt * BT, p.N, p.E, 1.0f);
        fv.template commit<false, true>(nullptr, vimg, kt * BT, p.N, p.E, 1.0f);
        const int nxt = min(kt + 1, nkt - 1) * BT;
        fk.fetch(kb, ld, nxt, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
        fv.fetch(vb, ld, nxt, p.N, p.E, nullptr, p.heads, head);
        __syncthreads();
        f32x4_t sacc[4];
        rows_times_frag_n<T, 4, HD>(sacc, kimg, s, g, qf);  // S^T[key = 16t + 4g + r][query = s]
        float pv[4][4];
        float mx = -INFINITY;
        if (kt * BT + BT <= p.N) {  // uniform: only the last tile of a sequence can hold padding keys
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pv[t][r] = sacc[t][r];
                    mx = fmaxf(mx, sacc[t][r]);
                }
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kt * BT + t * 16 + 4 * g + r;
                    const float v = key < p.N ? sacc[t][r] : -INFINITY;
                    pv[t][r] = v;
                    mx = fmaxf(mx, v);
                }
        }
        mx = group_max(mx);
        const float m_new = fmaxf(m_run, mx);
        const float mp = RowExp<T>::prep(m_new);
        const float alpha = RowExp<T>::sub(m_run, mp);
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = RowExp<T>::sub(pv[t][r], mp);
                psum += e;
                pv[t][r] = DROP ? (((mk[t] >> (8 * r)) & 0xffu) ? e * p.a_inv_keep : 0.f) : e;
            }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[dt][r] *= alpha;
        imgT_times_regs_n<T, 4, HD>(oacc, vimg, s, g, pv);  // O^T[d = 16dt + 4g + r][query = s]
    }
    const float l_tot = group_sum(l_run);
    const float inv = 1.0f / l_tot;
    {
        float ov[HD / 16][4];
#pragma unroll
        for (int dt = 0; dt < HD / 16; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) ov[dt][r] = oacc[dt][r] * inv;
        store_row<T, HD>(reinterpret_cast<T*>(p.o) + ((int64_t)b * p.N + min(q, p.N - 1)) * C + head * HD, ov, g, q < p.N);
        if (q < p.N && g == 0 && p.lse) p.lse[((int64_t)b * p.heads + head) * p.N + q] = m_run + logf(l_tot);
    }
}

// ---------------------------------------------------------------------------------
// backward, query side: delta, dq (and the q part of the cos gradient)
// ---------------------------------------------------------------------------------
template <typename T, int NW = 4, bool DROP = false, int HD = 64, bool ROT = false>
__global__ __launch_bounds__(64 * NW) void attn_bwd_dq_kernel(const AttnP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* kimg = smem;                                        // K~ rows     (AT<T, HD>::BWD_DQ_LDS bytes in all)
    unsigned char* vimg = smem + AT<T, HD>::ROW_IMG;                       // V rows
    unsigned char* ktr = smem + 2 * AT<T, HD>::ROW_IMG;                    // K~ transposed-read image
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const int qt = blockIdx.x % p.qtiles;
    const int bh = blockIdx.x / p.qtiles;
    const int head = bh % p.heads, b = bh / p.heads;
    if (p.nkeep && b >= *p.nkeep) return;  // compact rows: samples at or beyond the kept count are nobody's (before any staging)
    const int C = p.heads * HD;
    const int64_t ld = 3 * C;
    const T* qb = reinterpret_cast<const T*>(p.qkv) + (int64_t)b * p.N * ld + head * HD;
    const T* kb = qb + C;
    const T* vb = qb + 2 * C;
    const T* dob = reinterpret_cast<const T*>(p.d_o) + (int64_t)b * p.N * C + head * HD;
    const T* ob = reinterpret_cast<const T*>(p.o) + (int64_t)b * p.N * C + head * HD;
    const float scale = attn_scale<HD>();

    __shared__ float fl[HD];  // this workgroup's freqs-gradient partial [a][j]; zeroed here, published behind the loop's barriers
    float* fw = freq_wave_slot<HD>(p);
    if (threadIdx.x < HD) fl[threadIdx.x] = 0.f;
    const int q = qt * (16 * NW) + wave * 16 + s;
    uint4 qf[(AT<T, HD>::NKK)], dof[(AT<T, HD>::NKK)];
    load_row_frag<T, true, HD, ROT>(qf, qb, ld, q, p.N, p.E, g, p.cos_tab, p.heads, head, scale, p.sin_tab);
    load_row_frag<T, false, HD>(dof, dob, C, q, p.N, p.E, g, nullptr, p.heads, head, 1.0f);
    // delta = sum_d dO * O  (each lane holds 1/4 of the row)
    float dl = 0.f;
    {
        uint4 of[(AT<T, HD>::NKK)];
        load_row_frag<T, false, HD>(of, ob, C, q, p.N, p.E, g, nullptr, p.heads, head, 1.0f);
#pragma unroll
        for (int kk = 0; kk < AT<T, HD>::NKK; ++kk) {
            Vec16<T> a, bb;
            a.raw = dof[kk];
            bb.raw = of[kk];
#pragma unroll
            for (int j = 0; j < AT<T, HD>::EPV; ++j) dl += a.get(j) * bb.get(j);
        }
    }
    const float delta = group_sum(dl);
    const float lse_raw = p.lse[((int64_t)b * p.heads + head) * p.N + min(q, p.N - 1)];  // unconditional load, select after
    const float lse = RowExp<T>::prep(q < p.N ? lse_raw : 0.f);
    if (q < p.N && g == 0) p.delta[((int64_t)b * p.heads + head) * p.N + q] = delta;

    f32x4_t dq[HD / 16];
#pragma unroll
    for (int i = 0; i < HD / 16; ++i) dq[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const unsigned char* mrow = nullptr;
    if constexpr (DROP) mrow = p.amask + (((int64_t)b * p.heads + head) * p.N + min(q, p.N - 1)) * p.Np + 4 * g;

    const int nkt = (p.N + BT - 1) / BT;
    TileFetch<T, true, 64 * NW, HD, ROT> fk;   // the next key tile travels in registers while this one is multiplied
    TileFetch<T, false, 64 * NW, HD> fv;
    fk.fetch(kb, ld, 0, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
    fv.fetch(vb, ld, 0, p.N, p.E, nullptr, p.heads, head);
    for (int kt = 0; kt < nkt; ++kt) {
        uint32_t mk[4] = {0, 0, 0, 0};
        if constexpr (DROP) {
#pragma unroll
            for (int t = 0; t < 4; ++t) mk[t] = *reinterpret_cast<const uint32_t*>(mrow + kt * BT + 16 * t);
        }
        __syncthreads();
        fk.template commit<true, true>(kimg, ktr, kt * BT, p.N, p.E, 1.0f);
        fv.template commit<true, false>(vimg, nullptr, kt * BT, p.N, p.E, 1.0f);
        const int nxt = min(kt + 1, nkt - 1) * BT;
        fk.fetch(kb, ld, nxt, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
        fv.fetch(vb, ld, nxt, p.N, p.E, nullptr, p.heads, head);
        __syncthreads();
        // no masks: padding keys have zero rows in all three images (their finite dS meets a zero row of K~), padding queries
        // are not stored; the clamp keeps exp finite where (query, key) is not a real pair
        // two half steps of 32 keys: the same products with half the live registers (see the resident kernels)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4_t sacc[4], dpacc[4];
            rows_times_frag_n<T, 2, HD>(sacc, kimg + h * 32 * AT<T, HD>::ROWB, s, g, qf);    // S^T[key][q]
            PHASE_FENCE();
            rows_times_frag_n<T, 2, HD>(dpacc, vimg + h * 32 * AT<T, HD>::ROWB, s, g, dof);  // dP^T[key][q] = V[key] . dO[q]
            PHASE_FENCE();
            float ds[4][4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (t < 2) {
                        const float pr = RowExp<T>::clamped(sacc[t][r], lse);
                        const float dp = DROP ? (((mk[2 * h + t] >> (8 * r)) & 0xffu) ? dpacc[t][r] * p.a_inv_keep : 0.f) : dpacc[t][r];
                        ds[t][r] = pr * (dp - delta);
                    } else {
                        ds[t][r] = 0.f;
                    }
                }
            PHASE_FENCE();
            imgT_times_regs_n<T, 2, HD>(dq, ktr + h * 32 * AT<T, HD>::TRB, s, g, ds);  // dQ~^T[d][q] += K~^T . dS^T
            PHASE_FENCE();
        }
    }
    dq_epilogue<T, HD, ROT>(p, dq, qb, ld, b, head, q, s, g, scale, fl, fw);
    if (p.E < p.N) freq_flush<false, HD>(fl, p.fpart, p.fwave);
}

// ---------------------------------------------------------------------------------
// backward, key side: dk, dv (and the k part of the cos gradient)
// wave = 16 keys (lane s); loops over 64-query tiles
// ---------------------------------------------------------------------------------
// NW = 8: at least 4 waves per SIMD (two 8-wave workgroups per CU) -- left to itself the compiler takes 130 registers and
// only one workgroup fits
template <typename T, int NW = 4, bool DROP = false, int HD = 64, bool ROT = false>
__global__ __launch_bounds__(64 * NW, NW == 8 && HD == 64 ? 4 : 1) void attn_bwd_dkv_kernel(const AttnP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* qimg = smem;                                   // Q~ rows          (AT<T, HD>::BWD_DKV_LDS bytes in all)
    unsigned char* doimg = smem + AT<T, HD>::ROW_IMG;                 // dO rows
    unsigned char* qtr = smem + 2 * AT<T, HD>::ROW_IMG;               // Q~ transposed-read image
    unsigned char* dotr = qtr + AT<T, HD>::TR_IMG;                    // dO transposed-read image
    float* lse_s = reinterpret_cast<float*>(dotr + AT<T, HD>::TR_IMG);
    float* del_s = lse_s + BT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const int ktile = blockIdx.x % p.qtiles;  // same tiling for keys
    const int bh = blockIdx.x / p.qtiles;
    const int head = bh % p.heads, b = bh / p.heads;
    if (p.nkeep && b >= *p.nkeep) return;  // compact rows: samples at or beyond the kept count are nobody's (before any staging)
    const int C = p.heads * HD;
    const int64_t ld = 3 * C;
    const T* qb = reinterpret_cast<const T*>(p.qkv) + (int64_t)b * p.N * ld + head * HD;
    const T* kb = qb + C;
    const T* vb = qb + 2 * C;
    const T* dob = reinterpret_cast<const T*>(p.d_o) + (int64_t)b * p.N * C + head * HD;
    const float scale = attn_scale<HD>();
    const int64_t statbase = ((int64_t)b * p.heads + head) * p.N;

    __shared__ float fl[HD];
    float* fw = freq_wave_slot<HD>(p);
    if (threadIdx.x < HD) fl[threadIdx.x] = 0.f;
    const int key = ktile * (16 * NW) + wave * 16 + s;
    uint4 kf[(AT<T, HD>::NKK)], vf[(AT<T, HD>::NKK)];
    load_row_frag<T, true, HD, ROT>(kf, kb, ld, key, p.N, p.E, g, p.cos_tab, p.heads, head, 1.0f, p.sin_tab);
    load_row_frag<T, false, HD>(vf, vb, ld, key, p.N, p.E, g, nullptr, p.heads, head, 1.0f);

    f32x4_t dk[HD / 16], dv[HD / 16];
#pragma unroll
    for (int i = 0; i < HD / 16; ++i) {
        dk[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        dv[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const int nqt = (p.N + BT - 1) / BT;
    TileFetch<T, true, 64 * NW, HD, ROT> fq;   // the next query tile (and its statistics) travel in registers while this one is multiplied
    TileFetch<T, false, 64 * NW, HD> fdo;
    const int stl = threadIdx.x & (BT - 1);  // every thread fetches a statistic (unconditional load); the first 64 commit
    float l_n, d_n;
    fq.fetch(qb, ld, 0, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
    fdo.fetch(dob, C, 0, p.N, p.E, nullptr, p.heads, head);
    l_n = p.lse[statbase + min(stl, p.N - 1)];
    d_n = p.delta[statbase + min(stl, p.N - 1)];
    for (int qt = 0; qt < nqt; ++qt) {
        __syncthreads();
        fq.template commit<true, true>(qimg, qtr, qt * BT, p.N, p.E, scale);
        fdo.template commit<true, true>(doimg, dotr, qt * BT, p.N, p.E, 1.0f);
        if (threadIdx.x < BT) {
            const int qq = qt * BT + threadIdx.x;
            lse_s[threadIdx.x] = RowExp<T>::prep(qq < p.N ? l_n : 0.f);
            del_s[threadIdx.x] = qq < p.N ? d_n : 0.f;
        }
        const int nxt = min(qt + 1, nqt - 1) * BT;
        fq.fetch(qb, ld, nxt, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
        fdo.fetch(dob, C, nxt, p.N, p.E, nullptr, p.heads, head);
        l_n = p.lse[statbase + min(nxt + stl, p.N - 1)];
        d_n = p.delta[statbase + min(nxt + stl, p.N - 1)];
        __syncthreads();
        // no masks (see the dq kernel): padding queries have zero rows in the four images and finite statistics
#pragma unroll
        for (int h = 0; h < 2; ++h) {  // half steps of 32 queries
            f32x4_t sacc[4], dpacc[4];
            rows_times_frag_n<T, 2, HD>(sacc, qimg + h * 32 * AT<T, HD>::ROWB, s, g, kf);     // S[q = 16t + 4g + r][key = s]
            PHASE_FENCE();
            rows_times_frag_n<T, 2, HD>(dpacc, doimg + h * 32 * AT<T, HD>::ROWB, s, g, vf);   // dP[q][key]
            PHASE_FENCE();
            float pr[4][4], ds[4][4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (t < 2) {
                    const float4 l4 = *reinterpret_cast<const float4*>(lse_s + h * 32 + t * 16 + 4 * g);
                    const float4 d4 = *reinterpret_cast<const float4*>(del_s + h * 32 + t * 16 + 4 * g);
                    const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float pp = RowExp<T>::clamped(sacc[t][r], lv[r]);
                        float keepf = 1.0f;
                        if constexpr (DROP) {  // this lane's key, the tile's queries: one byte per (query, key)
                            const int qq = qt * BT + h * 32 + t * 16 + 4 * g + r;
                            keepf = p.amask[(((int64_t)b * p.heads + head) * p.N + min(qq, p.N - 1)) * p.Np + min(key, p.N - 1)] ? p.a_inv_keep : 0.f;
                        }
                        pr[t][r] = pp * keepf;
                        ds[t][r] = pp * (dpacc[t][r] * keepf - dvv[r]);
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pr[t][r] = ds[t][r] = 0.f;
                }
            }
            PHASE_FENCE();
            imgT_times_regs_n<T, 2, HD>(dv, dotr + h * 32 * AT<T, HD>::TRB, s, g, pr);  // dV^T[d][key] += dO^T . P
            PHASE_FENCE();
            imgT_times_regs_n<T, 2, HD>(dk, qtr + h * 32 * AT<T, HD>::TRB, s, g, ds);   // dK~^T[d][key] += Q~^T . dS
            PHASE_FENCE();
        }
    }
    dkv_epilogue<T, HD, ROT>(p, dk, dv, kb, ld, C, b, head, key, s, g, fl, fw);
    if (p.E < p.N) freq_flush<true, HD>(fl, p.fpart, p.fwave);
}

// ---------------------------------------------------------------------------------
// "Resident" variants for short sequences (N <= 256, bf16): one workgroup per (batch, head) stages
// the whole K~/V (forward, dq) or Q~/dO (dk/dv) of the head in LDS ONCE, then its waves walk their
// 16-row tiles with no barrier in the loop.  Against the tiled kernels above this removes the
// per-q-tile re-staging of K/V (4x at N = 199) and every in-loop __syncthreads.
// ---------------------------------------------------------------------------------
// One batch of a whole operand's staging: chunks i0, i0 + blockDim, ... (UN per thread) of the `total` 16-byte chunks of its image.
// Split like TileFetch: fetch() requests them (unconditional, clamped), commit() writes the images -- a kernel that stages several
// operands issues every fetch() before the first commit() and pays one memory round trip for all of them.
template <typename T, bool COS, bool ROT, int UN>
struct StageBatch {
    static constexpr int NCH = AT<T>::NCH, EPV = AT<T>::EPV;
    Chunk<T, COS, 64, ROT> ch[UN];
    __device__ __forceinline__ void fetch(const T* __restrict__ base, int64_t ld, int i0, int total, int N, int E, const float* __restrict__ cos_tab, int heads, int head,
                                          const float* __restrict__ sin_tab = nullptr) {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = min(i0 + u * (int)blockDim.x, total - 1);
            ch[u].fetch(base, ld, i / NCH, N, E, (i % NCH) * EPV, cos_tab, heads, head, sin_tab);
        }
    }
    template <bool ROWIMG, bool TRIMG>
    __device__ __forceinline__ void commit(unsigned char* rowimg, unsigned char* trimg, int i0, int total, int N, int E, float scale) const {
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = i0 + u * (int)blockDim.x;
            if (i < total) {
                const int r = i / NCH, c = i % NCH;
                const uint4 v = ch[u].value(r, N, E, scale);
                if constexpr (ROWIMG) st16(rowimg + r * AT<T>::ROWB + ((c ^ (r & AT<T>::SWZ)) << 4), v);
                if constexpr (TRIMG) st16(trimg + r * AT<T>::TRB + c * 16, v);
            }
        }
    }
};
template <typename T, bool COS, bool ROWIMG, bool TRIMG, bool ROT = false>
__device__ __forceinline__ void stage_all(unsigned char* rowimg, unsigned char* trimg, const T* __restrict__ base, int64_t ld, int nrows_pad, int N, int E,
                                          const float* __restrict__ cos_tab, int heads, int head, float scale, const float* __restrict__ sin_tab = nullptr) {
    constexpr int UN = 4;  // chunks in flight per thread (N <= 256: the whole operand in one batch of 512 threads)
    const int total = nrows_pad * AT<T>::NCH;
    for (int i0 = threadIdx.x; i0 < total; i0 += UN * blockDim.x) {
        StageBatch<T, COS, ROT, UN> sb;
        sb.fetch(base, ld, i0, total, N, E, cos_tab, heads, head, sin_tab);
        sb.template commit<ROWIMG, TRIMG>(rowimg, trimg, i0, total, N, E, scale);
    }
}

template <typename T, int NW = 8, bool ROT = false>  // NW = 4: sequences of at most 64 tokens (4 tiles of 16: half of an 8-wave workgroup would idle)
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_fwd_res_kernel(const AttnP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int HD = 64;  // the resident kernels carry head_dim 64 only
    const int nkt = (p.N + BT - 1) / BT;
    const int npad = nkt * BT;
    unsigned char* kimg = smem;  // res_fwd_lds<T>(npad) bytes in all
    unsigned char* vimg = smem + npad * AT<T>::ROWB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const int head = blockIdx.x % p.heads, b = blockIdx.x / p.heads;
    if (p.nkeep && b >= *p.nkeep) return;  // compact rows: samples at or beyond the kept count are nobody's (before any staging)
    const int C = p.heads * HD;
    const int64_t ld = 3 * C;
    const T* qb = reinterpret_cast<const T*>(p.qkv) + (int64_t)b * p.N * ld + head * HD;
    const T* kb = qb + C;
    const T* vb = qb + 2 * C;
    const float scale = 0.125f;
    stage_all<T, true, true, false, ROT>(kimg, nullptr, kb, ld, npad, p.N, p.E, p.cos_tab, p.heads, head, 1.0f, p.sin_tab);
    stage_all<T, false, false, true>(nullptr, vimg, vb, ld, npad, p.N, p.E, nullptr, p.heads, head, 1.0f);
    __syncthreads();
    const int nq16 = (p.N + 15) / 16;
    for (int qt = wave; qt < nq16; qt += NW) {
        const int q = qt * 16 + s;
        uint4 qf[AT<T>::NKK];
        load_row_frag<T, true, 64, ROT>(qf, qb, ld, q, p.N, p.E, g, p.cos_tab, p.heads, head, scale, p.sin_tab);
        f32x4_t oacc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) oacc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        float m_run = -INFINITY, l_run = 0.f;
        // NT live 16-key groups, MASK = the tile holds padding keys (only the last tile of a sequence can)
        auto kstep = [&](const int kt, auto ntc, auto maskc) __attribute__((always_inline)) {
            constexpr int NT = decltype(ntc)::value;
            constexpr bool MASK = decltype(maskc)::value != 0;
            f32x4_t sacc[4];
            rows_times_frag_n<T, NT>(sacc, kimg + kt * BT * AT<T>::ROWB, s, g, qf);
            float pv[4][4];
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float v = sacc[t][r];
                    if constexpr (MASK) v = kt * BT + t * 16 + 4 * g + r < p.N ? v : -INFINITY;
                    pv[t][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = group_max(mx);
            const float m_new = fmaxf(m_run, mx);
            const float mp = RowExp<T>::prep(m_new);
            const float alpha = RowExp<T>::sub(m_run, mp);
            float psum = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float e = t < NT ? RowExp<T>::sub(pv[t][r], mp) : 0.f;
                    pv[t][r] = e;
                    psum += e;
                }
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) oacc[dt][r] *= alpha;
            imgT_times_regs_n<T, NT>(oacc, vimg + kt * BT * AT<T>::TRB, s, g, pv);
        };
        const int nf = p.N / BT;  // tiles of 64 real keys
        for (int kt = 0; kt < nf; ++kt) kstep(kt, IC<4>{}, IC<0>{});
        if (nf < nkt) {
            if (p.N - nf * BT > 32) kstep(nf, IC<4>{}, IC<1>{});
            else kstep(nf, IC<2>{}, IC<1>{});
        }
        const float l_tot = group_sum(l_run);
        const float inv = 1.0f / l_tot;
        {
            float ov[4][4];
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[dt][r] = oacc[dt][r] * inv;
            store_row<T>(reinterpret_cast<T*>(p.o) + ((int64_t)b * p.N + min(q, p.N - 1)) * C + head * HD, ov, g, q < p.N);
            if (q < p.N && g == 0 && p.lse) p.lse[((int64_t)b * p.heads + head) * p.N + q] = m_run + logf(l_tot);
        }
    }
}

// ---- the pieces of the resident backward that attn_bwd_dq_res_kernel / attn_bwd_dkv_res_kernel (the pair) and attn_bwd_res_kernel
// (both phases in one workgroup) share: the same code, so the same arithmetic in the same order on either path ---------------------
// dq side, ahead of the key loop: the raw q values and (cos mode) the cos factors of the epilogue, requested with the tile's other fetches
template <typename T, bool ROT>
__device__ __forceinline__ void dq_res_prefetch(float (&qr)[4][4], float (&cr)[4][2], const AttnP& p, const T* __restrict__ qb, int64_t ld, int qc, int head, int g) {
    const T* qraw = qb + (int64_t)qc * ld;
    const float* cpr = p.cos_tab + ((int64_t)max(qc - p.E, 0) * p.heads + head) * 32;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const int d0 = dt * 16 + 4 * g;
        if constexpr (sizeof(T) == 2) {
            const uint2 r = *reinterpret_cast<const uint2*>(qraw + d0);
            const bf16_t* h = reinterpret_cast<const bf16_t*>(&r);
#pragma unroll
            for (int j = 0; j < 4; ++j) qr[dt][j] = (float)h[j];
        } else {
            const float4 r = *reinterpret_cast<const float4*>(qraw + d0);
            qr[dt][0] = r.x; qr[dt][1] = r.y; qr[dt][2] = r.z; qr[dt][3] = r.w;
        }
        if constexpr (!ROT) {  // (ROT: cos and sin are fetched behind the key loop, where the d-cos entries are fetched here)
            const float2 c2 = *reinterpret_cast<const float2*>(cpr + (d0 >> 1));
            cr[dt][0] = c2.x; cr[dt][1] = c2.y;
        }
    }
}
// dq of one 16-query wave tile over every staged key.
// No masks in the loop: the image rows of the padding keys (N <= key < npad) are zero, so whatever finite dS they
// get multiplies a zero row of K~; lanes of padding queries are not stored.  exp's argument is <= 0 for every real
// (query, key) pair, the clamp only keeps the padding ones finite.
// Steps of 32 keys (two 16-key groups, one MFMA contraction step of dS . K~): the images are staged in units of 32 rows,
// so every step is the same straight-line body -- and half the live registers of a 64-key step, which these kernels
// need (128-register budget).
template <typename T>
__device__ __forceinline__ void dq_res_loop(f32x4_t (&dq)[4], const unsigned char* kimg, const unsigned char* vimg, int npad, int s, int g,
                                            const uint4 (&qf)[AT<T>::NKK], const uint4 (&dof)[AT<T>::NKK], float lse, float delta) {
    for (int k0 = 0; k0 < npad; k0 += 32) {
        f32x4_t sacc[4], dpacc[4];
        rows_times_frag_pad_n<T, 2>(sacc, kimg + k0 * AT<T>::TRB, s, g, qf);
        PHASE_FENCE();
        rows_times_frag_pad_n<T, 2>(dpacc, vimg + k0 * AT<T>::TRB, s, g, dof);
        PHASE_FENCE();
        float ds[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) ds[t][r] = t < 2 ? RowExp<T>::clamped(sacc[t][r], lse) * (dpacc[t][r] - delta) : 0.f;
        PHASE_FENCE();
        imgT_times_regs_n<T, 2>(dq, kimg + k0 * AT<T>::TRB, s, g, ds);
        PHASE_FENCE();
    }
}
// dq epilogue of the resident kernels (qr, cr: dq_res_prefetch)
template <typename T, bool ROT>
__device__ __forceinline__ void dq_res_epilogue(const AttnP& p, const f32x4_t (&dq)[4], const float (&qr)[4][4], float (&cr)[4][2], int64_t ld, int b, int head, int q,
                                                int s, int g, float scale, float* fl, float* fw) {
    constexpr int HD = 64;
    const int qc = min(q, p.N - 1);
    const float* cpr = p.cos_tab + ((int64_t)max(qc - p.E, 0) * p.heads + head) * 32;
    // the d cos / d freqs table entries of this row: fetched here (after the key loop: held across it they would spill)
    const float* sxp = p.dsin + ((int64_t)max(qc - p.E, 0) * p.heads + head) * 32;
    const float* syp = sxp + (int64_t)(p.N - p.E) * p.heads * 32;
    float gp[4][2], dx[4][2], dy[4][2];
    float sr[ROT ? 4 : 1][2];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        if constexpr (ROT) {
            const float2 c2 = *reinterpret_cast<const float2*>(cpr + ((dt * 16 + 4 * g) >> 1));
            const float2 s2 = *reinterpret_cast<const float2*>(p.sin_tab + ((int64_t)max(qc - p.E, 0) * p.heads + head) * 32 + ((dt * 16 + 4 * g) >> 1));
            cr[dt][0] = c2.x; cr[dt][1] = c2.y;
            sr[dt][0] = s2.x; sr[dt][1] = s2.y;
            dx[dt][0] = dx[dt][1] = (float)(max(qc - p.E, 0) % p.W);
            dy[dt][0] = dy[dt][1] = (float)(max(qc - p.E, 0) / p.W);
            continue;
        }
        const float2 a = *reinterpret_cast<const float2*>(sxp + ((dt * 16 + 4 * g) >> 1));
        const float2 c = *reinterpret_cast<const float2*>(syp + ((dt * 16 + 4 * g) >> 1));
        dx[dt][0] = a.x; dx[dt][1] = a.y;
        dy[dt][0] = c.x; dy[dt][1] = c.y;
    }
    const bool row = q < p.N, img = row && q >= p.E;
    T* dqp = reinterpret_cast<T*>(p.dqkv) + ((int64_t)b * p.N + qc) * ld + head * HD;
    float oq[4][4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        if constexpr (ROT) {  // (see dq_epilogue)
            const float s0 = img ? sr[dt][0] : 0.f, s1 = img ? sr[dt][1] : 0.f, r0 = img ? cr[dt][0] : 1.0f, r1 = img ? cr[dt][1] : 1.0f;
            oq[dt][0] = scale * (dq[dt][0] * r0 + dq[dt][1] * s0); oq[dt][1] = scale * (dq[dt][1] * r0 - dq[dt][0] * s0);
            oq[dt][2] = scale * (dq[dt][2] * r1 + dq[dt][3] * s1); oq[dt][3] = scale * (dq[dt][3] * r1 - dq[dt][2] * s1);
            const float x0 = qr[dt][0] * r0 - qr[dt][1] * s0, x1 = qr[dt][0] * s0 + qr[dt][1] * r0;
            const float x2 = qr[dt][2] * r1 - qr[dt][3] * s1, x3 = qr[dt][2] * s1 + qr[dt][3] * r1;
            gp[dt][0] = img ? scale * (dq[dt][1] * x0 - dq[dt][0] * x1) : 0.f;
            gp[dt][1] = img ? scale * (dq[dt][3] * x2 - dq[dt][2] * x3) : 0.f;
            continue;
        }
        const float c0 = img ? cr[dt][0] * scale : scale, c1 = img ? cr[dt][1] * scale : scale;
        oq[dt][0] = dq[dt][0] * c0; oq[dt][1] = dq[dt][1] * c0; oq[dt][2] = dq[dt][2] * c1; oq[dt][3] = dq[dt][3] * c1;
        gp[dt][0] = img ? scale * (dq[dt][0] * qr[dt][0] + dq[dt][1] * qr[dt][1]) : 0.f;
        gp[dt][1] = img ? scale * (dq[dt][2] * qr[dt][2] + dq[dt][3] * qr[dt][3]) : 0.f;
    }
    store_row<T>(dqp, oq, g, row);
    if (p.E < p.N) freq_accum(fl, fw, gp, dx, dy, s, g);
}
// delta = rowsum(dO . O) of the lane's query: the four lanes g of a row each sum their chunks (kk, then the elements in order), then the group
template <typename T>
__device__ __forceinline__ float delta_of_row(const uint4 (&dof)[AT<T>::NKK], const uint4 (&of)[AT<T>::NKK]) {
    float dl = 0.f;
#pragma unroll
    for (int kk = 0; kk < AT<T>::NKK; ++kk) {
        Vec16<T> a, bb;
        a.raw = dof[kk];
        bb.raw = of[kk];
#pragma unroll
        for (int j = 0; j < AT<T>::EPV; ++j) dl += a.get(j) * bb.get(j);
    }
    return group_sum(dl);
}
// dk, dv of one 16-key wave tile over every staged query (lse_s: prepared LSE, del_s: delta, one entry per image row).
// No masks in the loop (see dq_res_loop): padding queries have zero rows in both images and finite statistics (0).
// steps of 32 queries (see dq_res_loop)
template <typename T>
__device__ __forceinline__ void dkv_res_loop(f32x4_t (&dk)[4], f32x4_t (&dv)[4], const unsigned char* qimg, const unsigned char* doimg, const float* lse_s,
                                             const float* del_s, int npad, int s, int g, const uint4 (&kf)[AT<T>::NKK], const uint4 (&vf)[AT<T>::NKK]) {
    for (int q0 = 0; q0 < npad; q0 += 32) {
        f32x4_t sacc[4], dpacc[4];
        rows_times_frag_pad_n<T, 2>(sacc, qimg + q0 * AT<T>::TRB, s, g, kf);
        PHASE_FENCE();
        rows_times_frag_pad_n<T, 2>(dpacc, doimg + q0 * AT<T>::TRB, s, g, vf);
        PHASE_FENCE();
        float pr[4][4], ds[4][4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (t < 2) {
                const float4 l4 = *reinterpret_cast<const float4*>(lse_s + q0 + t * 16 + 4 * g);
                const float4 d4 = *reinterpret_cast<const float4*>(del_s + q0 + t * 16 + 4 * g);
                const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dvv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pp = RowExp<T>::clamped(sacc[t][r], lv[r]);
                    pr[t][r] = pp;
                    ds[t][r] = pp * (dpacc[t][r] - dvv[r]);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) pr[t][r] = ds[t][r] = 0.f;
            }
        }
        PHASE_FENCE();
        imgT_times_regs_n<T, 2>(dv, doimg + q0 * AT<T>::TRB, s, g, pr);
        PHASE_FENCE();
        imgT_times_regs_n<T, 2>(dk, qimg + q0 * AT<T>::TRB, s, g, ds);
        PHASE_FENCE();
    }
}

template <typename T, int NW = 8, bool ROT = false>  // NW = 4: sequences of at most 64 tokens (4 tiles of 16: half of an 8-wave workgroup would idle)
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_bwd_dq_res_kernel(const AttnP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int HD = 64;  // the resident kernels carry head_dim 64 only
    const int nkt = (p.N + BT - 1) / BT;
    const int npad = (p.N + 31) & ~31;  // image rows: padding groups beyond it are never read (nt below)
    unsigned char* kimg = smem;         // padded-pitch images: row fragments AND transposed reads (res_bwd_dq_lds<T>(npad) bytes in all)
    unsigned char* vimg = kimg + npad * AT<T>::TRB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const int head = blockIdx.x % p.heads, b = blockIdx.x / p.heads;
    if (p.nkeep && b >= *p.nkeep) return;  // compact rows: samples at or beyond the kept count are nobody's (before any staging)
    const int C = p.heads * HD;
    const int64_t ld = 3 * C;
    const T* qb = reinterpret_cast<const T*>(p.qkv) + (int64_t)b * p.N * ld + head * HD;
    const T* kb = qb + C;
    const T* vb = qb + 2 * C;
    const T* dob = reinterpret_cast<const T*>(p.d_o) + (int64_t)b * p.N * C + head * HD;
    const T* ob = reinterpret_cast<const T*>(p.o) + (int64_t)b * p.N * C + head * HD;
    const float scale = 0.125f;
    __shared__ float fl[64];  // freqs-gradient partial of this (sample, head)
    float* fw = freq_wave_slot<64>(p);
    if (threadIdx.x < 64) fl[threadIdx.x] = 0.f;
    stage_all<T, true, false, true, ROT>(nullptr, kimg, kb, ld, npad, p.N, p.E, p.cos_tab, p.heads, head, 1.0f, p.sin_tab);
    stage_all<T, false, false, true>(nullptr, vimg, vb, ld, npad, p.N, p.E, nullptr, p.heads, head, 1.0f);
    __syncthreads();
    const int nq16 = (p.N + 15) / 16;
    for (int qt = wave; qt < nq16; qt += NW) {
        const int q = qt * 16 + s;
        // every fetch of a q tile in one batch (unconditional, clamped rows): q~, dO and O fragments, the raw q values
        // and cos factors of the epilogue, the row's LSE -- instead of one memory round trip per operand
        const int qc = min(q, p.N - 1);
        uint4 qf[AT<T>::NKK], dof[AT<T>::NKK];
        Chunk<T, true, 64, ROT> cq[AT<T>::NKK];
        Chunk<T, false> cdo[AT<T>::NKK], co[AT<T>::NKK];
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) {
            const int d0 = (kk * 4 + g) * AT<T>::EPV;
            cq[kk].fetch(qb, ld, q, p.N, p.E, d0, p.cos_tab, p.heads, head, p.sin_tab);
            cdo[kk].fetch(dob, C, q, p.N, p.E, d0, nullptr, p.heads, head);
            co[kk].fetch(ob, C, q, p.N, p.E, d0, nullptr, p.heads, head);
        }
        const float lse_raw = p.lse[((int64_t)b * p.heads + head) * p.N + qc];
        float qr[4][4], cr[4][2];
        dq_res_prefetch<T, ROT>(qr, cr, p, qb, ld, qc, head, g);
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) {
            qf[kk] = cq[kk].value(q, p.N, p.E, scale);
            dof[kk] = cdo[kk].value(q, p.N, p.E, 1.0f);
        }
        uint4 of[AT<T>::NKK];
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) of[kk] = co[kk].value(q, p.N, p.E, 1.0f);
        const float delta = delta_of_row<T>(dof, of);
        const float lse = RowExp<T>::prep(q < p.N ? lse_raw : 0.f);
        if (q < p.N && g == 0) p.delta[((int64_t)b * p.heads + head) * p.N + q] = delta;
        f32x4_t dq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dq[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        dq_res_loop<T>(dq, kimg, vimg, npad, s, g, qf, dof, lse, delta);
        dq_res_epilogue<T, ROT>(p, dq, qr, cr, ld, b, head, q, s, g, scale, fl, fw);
    }
    if (p.E < p.N) freq_flush<false>(fl, p.fpart, p.fwave);
}

// Diagnostic build only (-DATT_STAMP, tools/build_stamp.sh): per-phase s_memtime sums of wave 0 of one workgroup
#ifdef ATT_STAMP
__device__ unsigned long long g_att_stamp[8];
#define ATT_T(i) do { __builtin_amdgcn_sched_barrier(0); unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
                      __builtin_amdgcn_sched_barrier(0); tsum[i] += t_ - tlast; tlast = t_; } while (0)
#else
#define ATT_T(i) do { } while (0)
#endif

template <typename T, int NW = 8, bool ROT = false>  // NW = 4: sequences of at most 64 tokens (4 tiles of 16: half of an 8-wave workgroup would idle)
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_bwd_dkv_res_kernel(const AttnP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int HD = 64;  // the resident kernels carry head_dim 64 only
#ifdef ATT_STAMP
    unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tlast)::"memory");
#endif
    const int nqt = (p.N + BT - 1) / BT;
    const int npad = (p.N + 31) & ~31;
    unsigned char* qimg = smem;  // padded-pitch images: row fragments AND transposed reads (res_bwd_dkv_lds<T>(npad, nqt) bytes in all)
    unsigned char* doimg = qimg + npad * AT<T>::TRB;
    float* lse_s = reinterpret_cast<float*>(doimg + npad * AT<T>::TRB);
    float* del_s = lse_s + nqt * BT;  // statistics are indexed by every query slot of a 64-query tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const int head = blockIdx.x % p.heads, b = blockIdx.x / p.heads;
    if (p.nkeep && b >= *p.nkeep) return;  // compact rows: samples at or beyond the kept count are nobody's (before any staging)
    const int C = p.heads * HD;
    const int64_t ld = 3 * C;
    const T* qb = reinterpret_cast<const T*>(p.qkv) + (int64_t)b * p.N * ld + head * HD;
    const T* kb = qb + C;
    const T* vb = qb + 2 * C;
    const T* dob = reinterpret_cast<const T*>(p.d_o) + (int64_t)b * p.N * C + head * HD;
    const float scale = 0.125f;
    const int64_t statbase = ((int64_t)b * p.heads + head) * p.N;
    __shared__ float fl[64];  // freqs-gradient partial of this (sample, head)
    float* fw = freq_wave_slot<64>(p);
    if (threadIdx.x < 64) fl[threadIdx.x] = 0.f;
    stage_all<T, true, false, true, ROT>(nullptr, qimg, qb, ld, npad, p.N, p.E, p.cos_tab, p.heads, head, scale, p.sin_tab);
    stage_all<T, false, false, true>(nullptr, doimg, dob, C, npad, p.N, p.E, nullptr, p.heads, head, 1.0f);
    ATT_T(0);
    for (int i = threadIdx.x; i < nqt * BT; i += blockDim.x) {  // unconditional loads (clamped), zero by select
        const float l = p.lse[statbase + min(i, p.N - 1)], d = p.delta[statbase + min(i, p.N - 1)];
        lse_s[i] = RowExp<T>::prep(i < p.N ? l : 0.f);
        del_s[i] = i < p.N ? d : 0.f;
    }
    __syncthreads();
    ATT_T(1);
    const int nk16 = (p.N + 15) / 16;
    for (int ktile = wave; ktile < nk16; ktile += NW) {
        const int key = ktile * 16 + s;
        const int kc = min(key, p.N - 1);
        // every fetch of this key tile in one batch (see the dq kernel).  (Requesting the first tile's fragments before the
        // staging loads was tried in round 3: the chunks held across the staging spill, 212 -> 290 us for the pair of kernels.)
        uint4 kf[AT<T>::NKK], vf[AT<T>::NKK];
        Chunk<T, true, 64, ROT> ck[AT<T>::NKK];
        Chunk<T, false> cv[AT<T>::NKK];
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) {
            const int d0 = (kk * 4 + g) * AT<T>::EPV;
            ck[kk].fetch(kb, ld, key, p.N, p.E, d0, p.cos_tab, p.heads, head, p.sin_tab);
            cv[kk].fetch(vb, ld, key, p.N, p.E, d0, nullptr, p.heads, head);
        }
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) {
            kf[kk] = ck[kk].value(key, p.N, p.E, 1.0f);
            vf[kk] = cv[kk].value(key, p.N, p.E, 1.0f);
        }
        f32x4_t dk[4], dv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dk[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            dv[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        ATT_T(2);
        dkv_res_loop<T>(dk, dv, qimg, doimg, lse_s, del_s, npad, s, g, kf, vf);
        ATT_T(3);
        dkv_epilogue<T, 64, ROT>(p, dk, dv, kb, ld, C, b, head, key, s, g, fl, fw);
        ATT_T(4);
    }
    if (p.E < p.N) freq_flush<true>(fl, p.fpart, p.fwave);
#ifdef ATT_STAMP
    if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0)
        for (int i = 0; i < 8; ++i) g_att_stamp[i] = tsum[i];
#endif
}
#ifdef ATT_STAMP
extern "C" int lnx_dbg_attn_stamps(unsigned long long* out8) { return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_att_stamp), 64); }
#endif

// The whole resident backward of a (sample, head) in ONE workgroup, N <= 224: Q~, K~, V and dO are staged once (four padded-pitch
// images, 4 npad 160 bytes <= 140 KiB) and serve both phases, where the pair above stages two of them per kernel and fetches the other
// two per wave tile from global memory -- every operand read twice, two staging round trips, one fragment round trip per tile and
// `delta` through HBM.  One 16-row tile per wave per phase: NW = 4 for N <= 64, NW = 16 beyond.
//   delta   of every query first: q~ / dO fragments from the images (the bits Chunk::value gave the pair: the images hold exactly
//           those), O -- needed for delta only -- requested beside the staging loads; to LDS and to p.delta; one barrier
//   phase B (queries on the lane: attn_bwd_dq_res_kernel's body)   dq of the wave's query tile
//   phase A (keys on the lane: attn_bwd_dkv_res_kernel's body)     dk, dv of the wave's key tile; k~ / v fragments from the images
// No barrier between B and A.  The loops and epilogues are the pair's (dq_res_loop, dq_res_epilogue, dkv_res_loop, dkv_epilogue), so
// dqkv and delta are bit-equal to the pair's.  The freqs gradient is one LDS accumulator over both phases, published once
// (per_bh = 1 as for the pair).
// Image rows: the fragment reads take rows < 16 ntiles <= npad (N rounded up to 32), the loops rows < npad.  A wave whose tile lies
// beyond the sequence (N = 199: waves 13..15 for queries) stages, skips that phase and meets every barrier.
// Measured and not kept (stage-3 shape, B 256, N 199, 6 heads; the pair: 177-183 us): the phases behind one another with a barrier
// between them and no tile rotation, 162-168 us; that form as a persistent kernel (one workgroup per CU) that touches the next (sample,
// head)'s lines during phase A so that its staging finds them in L2, 170 us -- and holding the next problem's chunks in registers
// across a phase or an epilogue instead spills (116-174 registers).
template <typename T> constexpr size_t res_bwd_fused_lds(int npad, int qtiles) { return (size_t)npad * (4 * AT<T>::TRB) + (size_t)qtiles * BT * 2 * sizeof(float); }

template <typename T, int NW = 16, bool ROT = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(4, 4))) void attn_bwd_res_kernel(const AttnP p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int HD = 64;  // the resident kernels carry head_dim 64 only
#ifdef ATT_STAMP
    unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tlast)::"memory");
#endif
    constexpr int UN = 2;   // staging chunks per thread and operand: 8 npad <= 2 * 64 NW chunks (npad <= 64 at NW = 4, <= 256 at NW = 16)
    const int nqt = (p.N + BT - 1) / BT;
    const int npad = (p.N + 31) & ~31;
    unsigned char* qimg = smem;  // res_bwd_fused_lds<T>(npad, nqt) bytes in all
    unsigned char* kimg = qimg + npad * AT<T>::TRB;
    unsigned char* vimg = kimg + npad * AT<T>::TRB;
    unsigned char* doimg = vimg + npad * AT<T>::TRB;
    float* lse_s = reinterpret_cast<float*>(doimg + npad * AT<T>::TRB);
    float* del_s = lse_s + nqt * BT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = lane & 15, g = lane >> 4;
    const int head = blockIdx.x % p.heads, b = blockIdx.x / p.heads;
    if (p.nkeep && b >= *p.nkeep) return;  // compact rows: samples at or beyond the kept count are nobody's (before any staging)
    const int C = p.heads * HD;
    const int64_t ld = 3 * C;
    const T* qb = reinterpret_cast<const T*>(p.qkv) + (int64_t)b * p.N * ld + head * HD;
    const T* kb = qb + C;
    const T* vb = qb + 2 * C;
    const T* dob = reinterpret_cast<const T*>(p.d_o) + (int64_t)b * p.N * C + head * HD;
    const T* ob = reinterpret_cast<const T*>(p.o) + (int64_t)b * p.N * C + head * HD;
    const float scale = 0.125f;
    const int64_t statbase = ((int64_t)b * p.heads + head) * p.N;
    __shared__ float fl[64];  // freqs-gradient partial of this (sample, head), both phases
    float* fw = freq_wave_slot<64>(p);
    if (threadIdx.x < 64) fl[threadIdx.x] = 0.f;
    const int row = wave * 16 + s;  // the lane's query (delta, phase B)
    const int ntiles = (p.N + 15) / 16;
    const bool tile = wave < ntiles;
    Chunk<T, false> co[AT<T>::NKK];
    {
        // one memory round trip: every load of the four operands, the statistics and this wave's O fragment before the first wait
        const int total = npad * AT<T>::NCH, i0 = threadIdx.x;
        StageBatch<T, true, ROT, UN> sq, sk;
        StageBatch<T, false, false, UN> sv, sdo;
        sq.fetch(qb, ld, i0, total, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
        sk.fetch(kb, ld, i0, total, p.N, p.E, p.cos_tab, p.heads, head, p.sin_tab);
        sv.fetch(vb, ld, i0, total, p.N, p.E, nullptr, p.heads, head);
        sdo.fetch(dob, C, i0, total, p.N, p.E, nullptr, p.heads, head);
        const float l = p.lse[statbase + min(i0, p.N - 1)];  // nqt * BT <= 64 NW: one statistic slot per thread at the most
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) co[kk].fetch(ob, C, row, p.N, p.E, (kk * 4 + g) * AT<T>::EPV, nullptr, p.heads, head);
        sq.template commit<false, true>(nullptr, qimg, i0, total, p.N, p.E, scale);
        sk.template commit<false, true>(nullptr, kimg, i0, total, p.N, p.E, 1.0f);
        sv.template commit<false, true>(nullptr, vimg, i0, total, p.N, p.E, 1.0f);
        sdo.template commit<false, true>(nullptr, doimg, i0, total, p.N, p.E, 1.0f);
        if (i0 < nqt * BT) {
            lse_s[i0] = RowExp<T>::prep(i0 < p.N ? l : 0.f);
            del_s[i0] = 0.f;  // phase B fills the real queries' slots
        }
    }
    ATT_T(0);
    __syncthreads();
    ATT_T(1);
    // delta of every query first (cheap: two fragment reads and the O fragment), so that one barrier serves both phases and a wave
    // walks from its dq tile into its dk / dv tile without waiting for the others
    uint4 qf[AT<T>::NKK], dof[AT<T>::NKK];
    float delta = 0.f;
    if (tile) {
        uint4 of[AT<T>::NKK];
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) {  // (s, g) <- row, chunk kk * 4 + g: load_row_frag's mapping
            qf[kk] = ld16(qimg + row * AT<T>::TRB + ((kk * 4 + g) << 4));
            dof[kk] = ld16(doimg + row * AT<T>::TRB + ((kk * 4 + g) << 4));
            of[kk] = co[kk].value(row, p.N, p.E, 1.0f);
        }
        delta = delta_of_row<T>(dof, of);
        if (row < p.N && g == 0) {
            p.delta[statbase + row] = delta;
            del_s[row] = delta;
        }
    }
    ATT_T(2);
    __syncthreads();  // del_s complete
    ATT_T(3);
    if (tile) {  // ---- phase B: query tile `wave`
        const int q = row, qc = min(q, p.N - 1);
        float qr[4][4], cr[4][2];
        dq_res_prefetch<T, ROT>(qr, cr, p, qb, ld, qc, head, g);
        const float lse = lse_s[q];
        f32x4_t dq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dq[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        dq_res_loop<T>(dq, kimg, vimg, npad, s, g, qf, dof, lse, delta);
        ATT_T(4);
        dq_res_epilogue<T, ROT>(p, dq, qr, cr, ld, b, head, q, s, g, scale, fl, fw);
        ATT_T(5);
    }
    // ---- phase A: key tile (wave - ntiles % 4) mod NW.  Both loops keep their SIMD busy (the waves of a SIMD finish one after the
    // other, not together), so what counts is the tiles per SIMD over BOTH phases: with 13 tiles on 16 waves (wave w on SIMD w % 4)
    // SIMD 0 walks a fourth dq tile, and the rotation hands the fourth dk / dv tile to SIMD 1 -- 7, 7, 6, 6 instead of 8, 6, 6, 6.
    const int ktile = (wave + NW - ntiles % 4) % NW;
    if (ktile < ntiles) {
        const int key = ktile * 16 + s;
        uint4 kf[AT<T>::NKK], vf[AT<T>::NKK];
#pragma unroll
        for (int kk = 0; kk < AT<T>::NKK; ++kk) {
            kf[kk] = ld16(kimg + key * AT<T>::TRB + ((kk * 4 + g) << 4));
            vf[kk] = ld16(vimg + key * AT<T>::TRB + ((kk * 4 + g) << 4));
        }
        f32x4_t dk[4], dv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dk[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            dv[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        dkv_res_loop<T>(dk, dv, qimg, doimg, lse_s, del_s, npad, s, g, kf, vf);
        ATT_T(6);
        dkv_epilogue<T, 64, ROT>(p, dk, dv, kb, ld, C, b, head, key, s, g, fl, fw);
        ATT_T(7);
    }
    if (p.E < p.N) freq_flush<false>(fl, p.fpart, p.fwave);
#ifdef ATT_STAMP
    if (blockIdx.x == gridDim.x / 2 && threadIdx.x == 0)
        for (int i = 0; i < 8; ++i) g_att_stamp[i] = tsum[i];
#endif
}

// ---------------------------------------------------------------------------------
// cos table and its backward to the learnable freqs
// ---------------------------------------------------------------------------------
// HD / 2 frequencies per head: entry i = (n * heads + h) * HD / 2 + j
template <int HD = 64>
__device__ __forceinline__ void rope_cos_entry(const float* __restrict__ freqs, int heads, int H, int W, float* __restrict__ out, float* __restrict__ dsin, int i,
                                               float* __restrict__ sin_out = nullptr) {
    constexpr int HH = HD / 2, SH = HD == 32 ? 4 : HD == 64 ? 5 : 6;
    const int total = H * W * heads * HH;
    if (i >= total) return;
    const int j = i & (HH - 1);
    const int h = (i >> SH) % heads;
    const int n = (i >> SH) / heads;
    const float tx = (float)(n % W), ty = (float)(n / W);
    // theta = t_x * f_x + t_y * f_y in fp32, two rounded products then a rounded sum (einsum + add,
    // rope_2d_mhsa.py:136-142) -- keep them un-fused so the angle matches the reference bit for bit
    const float ax = __fmul_rn(tx, freqs[h * HH + j]);
    const float ay = __fmul_rn(ty, freqs[(heads + h) * HH + j]);
    const float th = __fadd_rn(ax, ay);
    out[i] = cosf(th);
    if (sin_out) sin_out[i] = sinf(th);  // LNX_ROPE_ROTATE: the imaginary part of polar(1, theta) (rope_2d_mhsa.py:143)
    if (dsin) {  // d cos(theta) / d freqs[a, h, j] = -t_a sin(theta): what the attention backward weights its pair gradients with
        const float ms = -sinf(th);
        dsin[i] = tx * ms;
        dsin[total + i] = ty * ms;
    }
}

template <int HD = 64>
__global__ __launch_bounds__(256) void rope_cos_kernel(const float* __restrict__ freqs, int heads, int H, int W, float* __restrict__ out,
                                                       float* __restrict__ dsin, float* __restrict__ sin_out) {
    rope_cos_entry<HD>(freqs, heads, H, W, out, dsin, blockIdx.x * 256 + threadIdx.x, sin_out);
}

// the tables of several blocks in one launch (every RoPE block of a plan has its own freqs): blockIdx.y picks the table.  One launch
// covers tables of one head_dim (the host groups them)
struct RopeTabBatch {
    lnx_rope_table t[LNX_ROPE_TABLES_MAX];
};
template <int HD = 64>
__global__ __launch_bounds__(256) void rope_cos_batch_kernel(const RopeTabBatch b) {
    const lnx_rope_table& t = b.t[blockIdx.y];
    rope_cos_entry<HD>(t.freqs, t.heads, t.H, t.W, t.cos_out, t.dsin_out, blockIdx.x * 256 + threadIdx.x, t.sin_out);
}

// dfreqs[a, h, j] += sum over the workgroups of head h of their partial [a][j]   (fixed order: deterministic given the partials)
// one 1024-thread workgroup per head: SL = 1024 / HD slices of the partial list x HD entries (16 x 64 at head_dim 64), four loads in
// flight per thread, LDS tree.  The one body of both fold kernels below: a call folded alone and in a batch gives the same bits.
template <int HD>
__device__ __forceinline__ void freqs_fold(const float* __restrict__ fpart, float* __restrict__ dfreqs, int B, int heads, int per_bh, int h, const int* nkeep) {
    constexpr int SL = 1024 / HD, HH = HD / 2;
    __shared__ float red[SL][HD];
    const int t = threadIdx.x & (HD - 1), sl = threadIdx.x / HD;  // t = a * HD / 2 + j
    if (nkeep) B = min(B, max(*nkeep, 0));  // compact rows: the skipped samples' workgroups wrote no partial (their slots hold anything)
    const int n = B * per_bh;  // partials of this head: (b, k) -> ((b * heads + h) * per_bh + k)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    auto at = [&](int i) -> float {
        const int ii = max(min(i, n - 1), 0);
        const int b = ii / per_bh, k = ii - b * per_bh;
        const float v = fpart[(((int64_t)b * heads + h) * per_bh + k) * HD + t];
        return i < n ? v : 0.f;
    };
    for (int i = sl; i < n; i += 4 * SL) {
        a0 += at(i);
        a1 += at(i + SL);
        a2 += at(i + 2 * SL);
        a3 += at(i + 3 * SL);
    }
    red[sl][t] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (sl == 0) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < SL; ++k) acc += red[k][t];
        dfreqs[((t / HH) * heads + h) * HH + (t & (HH - 1))] += acc;
    }
}
template <int HD = 64>
__global__ __launch_bounds__(1024) void rope_freqs_reduce_kernel(const float* __restrict__ fpart, int B, int heads, int per_bh, float* __restrict__ dfreqs,
                                                                 const int* nkeep) {
    freqs_fold<HD>(fpart, dfreqs, B, heads, per_bh, blockIdx.x, nkeep);
}

// the same fold for several attention backward calls in ONE launch (lnx_attn_bwd_args.defer_freqs + lnx_attn_bwd_flush): blockIdx.y picks
// the call.  Every RoPE block owns its freqs, so a backward segment of a plan has one of these small folds per block.  One launch folds
// the calls of one head_dim (freq_flush groups them).
struct FreqEntry {
    const float* fpart;
    float* dfreqs;
    int B, heads, per_bh, hd;
    const int* nkeep;
};
struct FreqBatch {
    FreqEntry e[LNX_ATTN_DEFER_MAX];
};
template <int HD = 64>
__global__ __launch_bounds__(1024) void rope_freqs_reduce_batch_kernel(const FreqBatch fb) {
    const FreqEntry& q = fb.e[blockIdx.y];
    if ((int)blockIdx.x >= q.heads) return;  // (uniform per workgroup: the grid's width is the largest head count of the batch)
    freqs_fold<HD>(q.fpart, q.dfreqs, q.B, q.heads, q.per_bh, blockIdx.x, q.nkeep);
}

// ---------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------
// f(IC<head_dim>{}) for a head_dim that passed hd_ok, and f(TC<element type>{}, IC<head_dim>{}): the only two places that turn the
// run-time head_dim / dtype of a call into template arguments
template <typename T> struct TC { using type = T; };
template <class F> auto with_hd(int hd, F&& f) {
    if (hd == 32) return f(IC<32>{});
    if (hd == 64) return f(IC<64>{});
    return f(IC<128>{});
}
template <class F> auto with_type_hd(int dtype, int hd, F&& f) {
    return with_hd(hd, [&](auto hdc) { return dtype == LNX_BF16 ? f(TC<bf16_t>{}, hdc) : f(TC<float>{}, hdc); });
}

// postponed folds of this thread's lnx_attn_bwd calls (raw pointers: the caller keeps partials and targets alive until the flush)
thread_local FreqEntry g_freq_pending[LNX_ATTN_DEFER_MAX];
thread_local int g_freq_n = 0;
thread_local hipStream_t g_freq_stream = nullptr;

int freq_flush(hipStream_t st) {
    if (g_freq_n == 0) return 0;
    LNX_CHECK(st == g_freq_stream, "lnx_attn_bwd_flush: the postponed folds belong to another stream");
    for (const int hd : {64, 32, 128}) {  // one launch per head_dim present (a plan of head_dim 64 only: the one launch it always made)
        FreqBatch fb{};
        int most = 0, m = 0;
        for (int i = 0; i < g_freq_n; ++i) {
            if (g_freq_pending[i].hd != hd) continue;
            fb.e[m] = g_freq_pending[i];
            if (fb.e[m].heads > most) most = fb.e[m].heads;
            ++m;
        }
        if (m == 0) continue;
        with_hd(hd, [&](auto hdc) { hipLaunchKernelGGL(rope_freqs_reduce_batch_kernel<decltype(hdc)::value>, dim3(most, m), dim3(1024), 0, st, fb); });
    }
    g_freq_n = 0;
    LNX_LAUNCH_CHECK();
    return 0;
}

// Every attention kernel is launched through here.  A kernel gets 64 KiB of dynamic LDS unasked; the limit of each instantiation is
// raised once, before its first launch and by whichever thread comes first (a function-local static: thread-safe), to `lds_max`, the
// most that instantiation is ever launched with -- so no list of "the ones beyond 64 KiB" has to follow the layouts.  If the runtime
// refused it, every launch of that instantiation reports the refusal (2, lnx_last_error) instead of launching.
template <auto Kernel>
int attn_launch(int grid, int block, size_t lds, size_t lds_max, hipStream_t st, const AttnP& p) {
    static const hipError_t raise_dynamic_lds_limit = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
    LNX_HIP(raise_dynamic_lds_limit);
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds, st, p);
    return 0;
}

bool hd_ok(int hd) { return hd == 32 || hd == 64 || hd == 128; }

// Without image tokens (E == N) a caller may pass no tables, yet the kernels fetch one entry of row 0 unconditionally (clamped
// rows, never used: only image tokens are scaled).  qkv (3 C elements per token) covers the C / 2 floats of such a fetch.
const float* cos_or_stub(const float* tab, const void* qkv) { return tab ? tab : reinterpret_cast<const float*>(qkv); }

int check_attn(int dtype, int B, int N, int E, int heads, int hd, const char* who) {
    LNX_CHECK(dtype == LNX_F32 || dtype == LNX_BF16, "%s: bad dtype %d", who, dtype);
    LNX_CHECK(B > 0 && N > 0 && heads > 0 && E >= 0 && E <= N, "%s: bad shape B=%d N=%d E=%d heads=%d", who, B, N, E, heads);
    LNX_CHECK(hd_ok(hd), "%s: head_dim %d is not supported (32, 64 or 128)", who, hd);
    return 0;
}

// tiled bf16 kernels: 8 waves (128 rows) per workgroup for sequences beyond the resident kernels' reach, where every staged
// tile is then shared by twice the rows; 4 waves for short ones (more workgroups) and with LNX_ATTN_NW=4 (A/B switch)
static bool tiled_nw8(int N) {
    static const bool force4 = getenv("LNX_ATTN_NW") != nullptr && atoi(getenv("LNX_ATTN_NW")) == 4;
    return !force4 && N > 128;
}

// The tiled kernels exist with NW = 8 for bf16 at head_dim 64 and 128 only.  bf16 head_dim 32 keeps NW = 4 throughout: a 64-row tile
// is 256 16-byte chunks, one per thread of 4 waves.
template <typename T, int HD> constexpr bool hd_nw8() { return sizeof(T) == 2 && HD > 32; }

// The kernel family of a forward / backward launch (include/lnx.h: lnx_attn_dispatch answers with this, lnx_attn_fwd / lnx_attn_bwd
// launch by it).  Arguments already passed check_attn.
int attn_family(int dtype, int N, int hd, bool drop) {
    if (dtype != LNX_BF16 || drop || hd == 32) return LNX_ATTN_KERNEL_TILED4;
    if (hd == 64 && N <= 256 && getenv("LNX_ATTN_TILED") == nullptr) return N <= 64 ? LNX_ATTN_KERNEL_RES4 : LNX_ATTN_KERNEL_RES8;
    return tiled_nw8(N) ? LNX_ATTN_KERNEL_TILED8 : LNX_ATTN_KERNEL_TILED4;
}
bool is_resident(int family) { return family == LNX_ATTN_KERNEL_RES4 || family == LNX_ATTN_KERNEL_RES8; }

std::atomic<int> g_last_attn{LNX_ATTN_KERNEL_NONE};

// ---- the tiled kernels (any dtype and head_dim).  The whole rule for their instantiation: a dropout mask -> NW = 4 with the DROP code;
// LNX_ATTN_KERNEL_TILED8 -> NW = 8; everything else NW = 4.  f(IC<NW>{}, IC<DROP>{}) launches; p.qtiles becomes the workgroups per
// (sample, head) of that NW (p.Np keeps the 64-row rounding of the mask).
template <typename T, int HD, class F>
int tiled_variant(AttnP& p, int family, F&& f) {
    if (p.amask) return f(IC<4>{}, IC<1>{});
    if constexpr (hd_nw8<T, HD>()) {
        if (family == LNX_ATTN_KERNEL_TILED8) {
            p.qtiles = cdiv(p.N, 128);
            return f(IC<8>{}, IC<0>{});
        }
    }
    return f(IC<4>{}, IC<0>{});
}

template <typename T, int HD, bool ROT>
int attn_fwd_tiled(AttnP& p, int family, hipStream_t st) {
    return tiled_variant<T, HD>(p, family, [&](auto nwc, auto dropc) {
        constexpr int NW = decltype(nwc)::value;
        constexpr bool DROP = decltype(dropc)::value != 0;
        constexpr size_t lds = AT<T, HD>::FWD_LDS;
        return attn_launch<attn_fwd_kernel<T, NW, DROP, HD, ROT>>(p.B * p.heads * p.qtiles, 64 * NW, lds, lds, st, p);
    });
}

// the backward launchers leave the workgroups per (sample, head) of their launches in per_bh (what the freqs fold needs)
template <typename T, int HD, bool ROT>
int attn_bwd_tiled(AttnP& p, int family, hipStream_t st, int& per_bh) {
    return tiled_variant<T, HD>(p, family, [&](auto nwc, auto dropc) {
        constexpr int NW = decltype(nwc)::value;
        constexpr bool DROP = decltype(dropc)::value != 0;
        constexpr size_t lds_q = AT<T, HD>::BWD_DQ_LDS, lds_k = AT<T, HD>::BWD_DKV_LDS;
        const int grid = p.B * p.heads * p.qtiles;
        per_bh = p.qtiles;
        if (int rc = attn_launch<attn_bwd_dq_kernel<T, NW, DROP, HD, ROT>>(grid, 64 * NW, lds_q, lds_q, st, p)) return rc;
        return attn_launch<attn_bwd_dkv_kernel<T, NW, DROP, HD, ROT>>(grid, 64 * NW, lds_k, lds_k, st, p);
    });
}

// ---- the resident kernels (bf16, head_dim 64, N <= 256): one workgroup per (sample, head), NW = 4 up to 64 tokens
// (LNX_ATTN_KERNEL_RES4) and 8 beyond (RES8).  f(IC<NW>{}, the longest sequence of that NW) launches.
template <class F>
int res_variant(int family, F&& f) {
    return family == LNX_ATTN_KERNEL_RES4 ? f(IC<4>{}, 64) : f(IC<8>{}, 256);
}

template <bool ROT>
int attn_fwd_res(AttnP& p, int family, hipStream_t st) {
    typedef bf16_t T;
    return res_variant(family, [&](auto nwc, int nmax) {
        constexpr int NW = decltype(nwc)::value;
        return attn_launch<attn_fwd_res_kernel<T, NW, ROT>>(p.B * p.heads, 64 * NW, res_fwd_lds<T>(p.qtiles * BT), res_fwd_lds<T>(nmax), st, p);
    });
}

// Backward: N <= 224 runs attn_bwd_res_kernel (one launch: 4 waves for LNX_ATTN_KERNEL_RES4, 16 for RES8 -- the family names the
// forward's waves); 225..256, where four images no longer fit the 160 KiB of LDS, and any N with LNX_ATTN_BWD_SPLIT in the
// environment (read per call: the A/B switch) run the dq / dk-dv pair.  g_last_bwd_launches: what lnx_last_attn_bwd_launches reports.
constexpr int RES_BWD_FUSED_NMAX = 224;
std::atomic<int> g_last_bwd_launches{0};

template <bool ROT>
int attn_bwd_res(AttnP& p, int family, hipStream_t st, int& per_bh) {
    typedef bf16_t T;
    const int npad = (p.N + 31) & ~31, bh = p.B * p.heads;
    per_bh = 1;
    if (p.N <= RES_BWD_FUSED_NMAX && getenv("LNX_ATTN_BWD_SPLIT") == nullptr) {
        g_last_bwd_launches.store(1, std::memory_order_relaxed);
        const size_t lds = res_bwd_fused_lds<T>(npad, p.qtiles);
        if (family == LNX_ATTN_KERNEL_RES4) return attn_launch<attn_bwd_res_kernel<T, 4, ROT>>(bh, 64 * 4, lds, res_bwd_fused_lds<T>(64, 1), st, p);
        return attn_launch<attn_bwd_res_kernel<T, 16, ROT>>(bh, 64 * 16, lds, res_bwd_fused_lds<T>(RES_BWD_FUSED_NMAX, cdiv(RES_BWD_FUSED_NMAX, BT)), st, p);
    }
    return res_variant(family, [&](auto nwc, int nmax) {
        constexpr int NW = decltype(nwc)::value;
        if (int rc = attn_launch<attn_bwd_dq_res_kernel<T, NW, ROT>>(bh, 64 * NW, res_bwd_dq_lds<T>(npad), res_bwd_dq_lds<T>(nmax), st, p)) return rc;
        return attn_launch<attn_bwd_dkv_res_kernel<T, NW, ROT>>(bh, 64 * NW, res_bwd_dkv_lds<T>(npad, p.qtiles), res_bwd_dkv_lds<T>(nmax, nmax / BT), st, p);
    });
}

int rope_table_hd(const float* freqs, int heads, int hd, int H, int W, float* cos_out, float* dsin_out, hipStream_t st, const char* who, float* sin_out = nullptr) {
    LNX_CHECK(freqs && cos_out && heads > 0 && H > 0 && W > 0, "%s: bad arguments", who);
    LNX_CHECK(hd_ok(hd), "%s: head_dim %d is not supported (32, 64 or 128)", who, hd);
    const int total = H * W * heads * (hd / 2);
    with_hd(hd, [&](auto hdc) {
        hipLaunchKernelGGL(rope_cos_kernel<decltype(hdc)::value>, dim3(cdiv(total, 256)), dim3(256), 0, st, freqs, heads, H, W, cos_out, dsin_out, sin_out);
    });
    LNX_LAUNCH_CHECK();
    return 0;
}

// What lnx_attn_fwd and lnx_attn_bwd share once their own argument checks have passed: the dropout arguments (the last check of a
// call: nothing has been launched or recorded before it), the fields of AttnP that both directions fill, and the choice of the kernel
// family, which lnx_last_attn_kernel reports from here on.  Args = lnx_attn_args or lnx_attn_bwd_args.
template <bool ROT, class Args>
int attn_setup(const Args* a, const int* nkeep, int hd, const char* who, AttnP& p, int& family) {
    if (a->drop_mask) {  // attention-probability dropout: the 64-row tiled kernels with the DROP code
        LNX_CHECK(a->drop_inv_keep >= 1.0f && (((uintptr_t)a->drop_mask) & 3) == 0, "%s: drop_inv_keep >= 1 and a 4-byte aligned mask", who);
    }
    p.qkv = a->qkv; p.cos_tab = cos_or_stub(a->cos_tab, a->qkv); p.o = const_cast<void*>(static_cast<const void*>(a->o)); p.lse = const_cast<float*>(a->lse);
    if (ROT) p.sin_tab = cos_or_stub(a->sin_tab, a->qkv);
    p.B = a->B; p.N = a->N; p.E = a->E; p.heads = a->heads;
    p.nkeep = nkeep;
    LNX_CHECK(!(nkeep && a->drop_mask), "%s: nkeep (compact rows) and the attention-probability mask (laid out by full rows) do not go together", who);
    p.qtiles = cdiv(a->N, BT);
    if (a->drop_mask) {
        p.amask = a->drop_mask; p.a_inv_keep = a->drop_inv_keep; p.Np = p.qtiles * BT;
    }
    family = attn_family(a->dtype, a->N, hd, a->drop_mask != nullptr);
    g_last_attn.store(family, std::memory_order_relaxed);
    return 0;
}

}  // namespace

extern "C" int lnx_rope_cos_table(const float* freqs, int heads, int H, int W, float* cos_out, float* dsin_out, void* stream) {
    return rope_table_hd(freqs, heads, 64, H, W, cos_out, dsin_out, (hipStream_t)stream, "lnx_rope_cos_table");
}

extern "C" int lnx_rope_cos_table_hd(const float* freqs, int heads, int head_dim, int H, int W, float* cos_out, float* dsin_out, void* stream) {
    return rope_table_hd(freqs, heads, head_dim, H, W, cos_out, dsin_out, (hipStream_t)stream, "lnx_rope_cos_table_hd");
}

extern "C" int lnx_rope_cossin_table_hd(const float* freqs, int heads, int head_dim, int H, int W, float* cos_out, float* sin_out, float* dsin_out, void* stream) {
    return rope_table_hd(freqs, heads, head_dim, H, W, cos_out, dsin_out, (hipStream_t)stream, "lnx_rope_cossin_table_hd", sin_out);
}

extern "C" int lnx_rope_cos_tables(const lnx_rope_table* t, int n, void* stream) {
    LNX_CHECK(t && n > 0, "lnx_rope_cos_tables: bad arguments");
    for (int i = 0; i < n; ++i) LNX_CHECK(t[i].freqs && t[i].cos_out && t[i].heads > 0 && t[i].H > 0 && t[i].W > 0, "lnx_rope_cos_tables: bad table");
    for (int i = 0; i < n; ++i)
        LNX_CHECK(t[i].head_dim == 0 || hd_ok(t[i].head_dim), "lnx_rope_cos_tables: head_dim %d is not supported (32, 64 or 128)", t[i].head_dim);
    for (int i = 0; i < n; ++i) {
        LNX_CHECK(t[i].rope_mode == LNX_ROPE_COS || t[i].rope_mode == LNX_ROPE_ROTATE, "lnx_rope_cos_tables: bad rope_mode %d", t[i].rope_mode);
        LNX_CHECK(t[i].rope_mode != LNX_ROPE_ROTATE || t[i].sin_out, "lnx_rope_cos_tables: a LNX_ROPE_ROTATE table needs sin_out");
    }
    for (const int hd : {64, 32, 128}) {  // one launch (per LNX_ROPE_TABLES_MAX tables) per head_dim present, tables in their order
        std::vector<lnx_rope_table> g;
        for (int i = 0; i < n; ++i)
            if ((t[i].head_dim ? t[i].head_dim : 64) == hd) g.push_back(t[i]);
        const int ng = (int)g.size();
        for (int i0 = 0; i0 < ng; i0 += LNX_ROPE_TABLES_MAX) {
            RopeTabBatch b{};
            const int m = ng - i0 < LNX_ROPE_TABLES_MAX ? ng - i0 : LNX_ROPE_TABLES_MAX;
            int most = 0;
            for (int i = 0; i < m; ++i) {
                b.t[i] = g[i0 + i];
                const int total = g[i0 + i].H * g[i0 + i].W * g[i0 + i].heads * (hd / 2);
                if (total > most) most = total;
            }
            with_hd(hd, [&](auto hdc) {
                hipLaunchKernelGGL(rope_cos_batch_kernel<decltype(hdc)::value>, dim3(cdiv(most, 256), m), dim3(256), 0, (hipStream_t)stream, b);
            });
            LNX_LAUNCH_CHECK();
        }
    }
    return 0;
}

// floats of lnx_attn_bwd's freqs-gradient workspace: one [2][head_dim / 2] partial per workgroup of its finest tiling
// (deterministic mode: behind them, FREQ_WAVES per-wave slots of the same shape per workgroup -- freq_accum)
extern "C" int64_t lnx_attn_bwd_ws_floats_hd(int B, int N, int heads, int head_dim) {
    return hd_ok(head_dim) ? (int64_t)B * heads * cdiv(N, BT) * head_dim * (deterministic() ? 1 + FREQ_WAVES : 1) : 0;
}
extern "C" int64_t lnx_attn_bwd_ws_floats(int B, int N, int heads) { return lnx_attn_bwd_ws_floats_hd(B, N, heads, 64); }

// ROT = the call's rope_mode is LNX_ROPE_ROTATE: the same families and launch shapes, the rotating instantiations
template <bool ROT>
int attn_fwd_launch(const lnx_attn_args* a, const int* nkeep, void* stream) {
    const int hd = a->head_dim ? a->head_dim : 64;
    if (check_attn(a->dtype, a->B, a->N, a->E, a->heads, hd, "lnx_attn_fwd")) return 1;
    LNX_CHECK(a->E == a->N || a->cos_tab, "lnx_attn_fwd: cos table missing");
    LNX_CHECK(!ROT || a->E == a->N || a->sin_tab, "lnx_attn_fwd: sin table missing (rope_mode = LNX_ROPE_ROTATE)");
    AttnP p{};
    int family = LNX_ATTN_KERNEL_NONE;
    if (attn_setup<ROT>(a, nkeep, hd, "lnx_attn_fwd", p, family)) return 1;
    hipStream_t st = (hipStream_t)stream;
    const int rc = is_resident(family) ? attn_fwd_res<ROT>(p, family, st) : with_type_hd(a->dtype, hd, [&](auto tc, auto hdc) {
        return attn_fwd_tiled<typename decltype(tc)::type, decltype(hdc)::value, ROT>(p, family, st);
    });
    if (rc) return rc;
    LNX_LAUNCH_CHECK();
    return 0;
}

template <bool ROT>
int attn_bwd_launch(const lnx_attn_bwd_args* a, const int* nkeep, int64_t freq_ws_floats, void* stream) {
    const int hd = a->head_dim ? a->head_dim : 64;
    if (check_attn(a->dtype, a->B, a->N, a->E, a->heads, hd, "lnx_attn_bwd")) return 1;
    if (ROT) {
        LNX_CHECK(a->E == a->N || (a->cos_tab && a->sin_tab && a->freq_ws && a->dfreqs), "lnx_attn_bwd: cos / sin tables, freqs-gradient workspace or dfreqs missing");
        LNX_CHECK(a->E == a->N || (a->grid_w > 0 && (a->N - a->E) % a->grid_w == 0), "lnx_attn_bwd: grid_w %d does not divide the %d image tokens", a->grid_w, a->N - a->E);
    } else {
        LNX_CHECK(a->E == a->N || (a->cos_tab && a->dsin_tab && a->freq_ws && a->dfreqs), "lnx_attn_bwd: cos / d-cos tables, freqs-gradient workspace or dfreqs missing");
    }
    hipStream_t st = (hipStream_t)stream;
    if (a->defer_freqs && a->E < a->N) {  // checked before anything is launched
        LNX_CHECK(g_freq_n == 0 || g_freq_stream == st, "lnx_attn_bwd: postponed freqs folds are pending on another stream (lnx_attn_bwd_flush them first)");
        LNX_CHECK(g_freq_n < LNX_ATTN_DEFER_MAX, "lnx_attn_bwd: %d postponed freqs folds are pending; call lnx_attn_bwd_flush", LNX_ATTN_DEFER_MAX);
    }
    AttnP p{};
    int family = LNX_ATTN_KERNEL_NONE;
    if (attn_setup<ROT>(a, nkeep, hd, "lnx_attn_bwd", p, family)) return 1;
    if (ROT) p.W = a->grid_w > 0 ? a->grid_w : 1;
    if (deterministic() && a->E < a->N) {
        const int64_t partials = (int64_t)a->B * a->heads * cdiv(a->N, BT) * hd, need = partials * (1 + FREQ_WAVES);
        LNX_CHECK(freq_ws_floats >= need,
                  "lnx_attn_bwd: deterministic mode needs lnx_attn_bwd_sized with freq_ws_floats >= lnx_attn_bwd_ws_floats_hd(...) = %lld floats with the mode "
                  "on (got %lld): the waves' slots lie behind the workgroups' partials", (long long)need, (long long)freq_ws_floats);
        p.fwave = a->freq_ws + partials;
    }
    p.d_o = a->d_o; p.dqkv = a->dqkv; p.fpart = a->freq_ws; p.dsin = cos_or_stub(a->dsin_tab, a->qkv); p.delta = a->delta;
    int per_bh = 0;
    g_last_bwd_launches.store(2, std::memory_order_relaxed);  // every path but the one-kernel resident backward
    const int rc = is_resident(family) ? attn_bwd_res<ROT>(p, family, st, per_bh) : with_type_hd(a->dtype, hd, [&](auto tc, auto hdc) {
        return attn_bwd_tiled<typename decltype(tc)::type, decltype(hdc)::value, ROT>(p, family, st, per_bh);
    });
    if (rc) return rc;
    // after the two kernels: the per-workgroup partials of the freqs gradient -> dfreqs (per_bh = workgroups per (sample, head))
    if (a->E < a->N) {
        if (a->defer_freqs) {
            g_freq_pending[g_freq_n++] = FreqEntry{p.fpart, a->dfreqs, a->B, a->heads, per_bh, hd, nkeep};
            g_freq_stream = st;
        } else {
            with_hd(hd, [&](auto hdc) {
                hipLaunchKernelGGL(rope_freqs_reduce_kernel<decltype(hdc)::value>, dim3(a->heads), dim3(1024), 0, st, p.fpart, a->B, a->heads, per_bh, a->dfreqs, nkeep);
            });
        }
    }
    LNX_LAUNCH_CHECK();
    return 0;
}

extern "C" int lnx_attn_fwd_compact(const lnx_attn_args* a, const int* nkeep, void* stream) {
    LNX_CHECK(a && a->qkv && a->o, "lnx_attn_fwd: null operand");
    LNX_CHECK(a->rope_mode == LNX_ROPE_COS || a->rope_mode == LNX_ROPE_ROTATE, "lnx_attn_fwd: bad rope_mode %d", a->rope_mode);
    return a->rope_mode == LNX_ROPE_ROTATE ? attn_fwd_launch<true>(a, nkeep, stream) : attn_fwd_launch<false>(a, nkeep, stream);
}
extern "C" int lnx_attn_fwd(const lnx_attn_args* a, void* stream) { return lnx_attn_fwd_compact(a, nullptr, stream); }

extern "C" int lnx_attn_bwd_compact(const lnx_attn_bwd_args* a, const int* nkeep, int64_t freq_ws_floats, void* stream) {
    LNX_CHECK(a && a->qkv && a->o && a->lse && a->d_o && a->dqkv && a->delta, "lnx_attn_bwd: null operand");
    LNX_CHECK(a->rope_mode == LNX_ROPE_COS || a->rope_mode == LNX_ROPE_ROTATE, "lnx_attn_bwd: bad rope_mode %d", a->rope_mode);
    return a->rope_mode == LNX_ROPE_ROTATE ? attn_bwd_launch<true>(a, nkeep, freq_ws_floats, stream) : attn_bwd_launch<false>(a, nkeep, freq_ws_floats, stream);
}
extern "C" int lnx_attn_bwd_sized(const lnx_attn_bwd_args* a, int64_t freq_ws_floats, void* stream) { return lnx_attn_bwd_compact(a, nullptr, freq_ws_floats, stream); }

extern "C" int lnx_attn_bwd(const lnx_attn_bwd_args* a, void* stream) { return lnx_attn_bwd_sized(a, 0, stream); }

extern "C" int lnx_attn_dispatch(int dtype, int N, int head_dim, int has_drop_mask) {
    const int hd = head_dim ? head_dim : 64;
    if ((dtype != LNX_F32 && dtype != LNX_BF16) || N <= 0 || !hd_ok(hd)) return -1;
    return attn_family(dtype, N, hd, has_drop_mask != 0);
}

extern "C" int lnx_last_attn_kernel(void) { return g_last_attn.load(std::memory_order_relaxed); }

extern "C" int lnx_last_attn_bwd_launches(void) { return g_last_bwd_launches.load(std::memory_order_relaxed); }

extern "C" int lnx_attn_bwd_flush(void* stream) { return freq_flush((hipStream_t)stream); }

extern "C" int lnx_attn_bwd_discard(void) {
    const int n = g_freq_n;
    g_freq_n = 0;
    return n;
}
