// gemm_nt v9 (round 4): the 256x256 / BK = 32 / four-stage ring / ping-pong K loop of gemm_nt_v4 as a PERSISTENT kernel that draws
// its tiles from the per-XCD atomic counters (common.hpp) and never lets the ring drain.
//
// Why.  One-shot gemm_nt_v4 spends a quarter of a tile's life outside the K loop at K = 1024: the first three slices'
// round trip at the start (one workgroup per CU: nothing else runs meanwhile) and the epilogue at the end.  Here the last three K
// iterations of a tile fetch the NEXT tile's first three slices, so the prologue latency disappears under the epilogue, and the
// epilogue's stores drain under the first two iterations of the next tile: stores, LDS-DMA and loads share one in-order counter,
// so those two iterations wait with the stores' count added (a compile-time number for a full tile; a partial last row tile
// drains instead), i.e. for "slice k+1 landed" and not for "every store acknowledged".  What v9 does NOT do is gemm_nt_v7's
// deferral of the stores into the next K loop: a 128x64 wave tile's results are 64-128 registers on top of 128 accumulator registers,
// which the 256-register budget of two waves per SIMD does not hold (v7's 64x64 wave tiles do).
//
// Scheduling: the draw protocol of common.hpp, as gemm_nt_v7 -- wave 0 draws the position after next in iteration 0 (one more operation on ITS counter), publishes it
// through an LDS dword in iteration 2, everyone reads it in iteration 3; first use in iteration nk - 3 >= 5.  K / 32 >= 8.
#include "gemm_common.hpp"

namespace lnxg {

// 16-byte stores one lane issues in the epilogue of a FULL tile (two 64x64 sub-tiles): what the first two iterations of the next
// tile let stay in flight.  Checked against the compiled code by tools/audit_counted_waits.py
// (run by __graft_entry__.build() and tests/test_host_logic.py: a mismatch fails the build; a smaller number is always safe).
template <bool OUT_F32, int F> struct EpiStores {
    static constexpr int value = 2 * (OUT_F32 ? 16 : 8) + ((F & F_C2) ? 16 : 0);
};

template <bool OUT_F32, int F>
__global__ __launch_bounds__(512) void gemm_nt_v9_kernel(const GemmP p_host) {
    typedef bf16_t T;
    typedef WideRing R;
    GemmP p = p_host;
    effective_rows_persistent<R::BM>(p);  // m_dev: the tile total, the row clamps and the store masks all come from the effective M
    if (p.M <= 0) return;                 // (nobody draws: the counters stay at zero)
    constexpr int NSTORE = EpiStores<OUT_F32, F>::value;
    static_assert(2 * R::PIECES + NSTORE + 1 <= 63, "vmcnt is a 6-bit counter");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];  // [R::NST][A 256 rows | W 256 rows][64 B] + one dword

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;  // waves 0-3 / 4-7 (the ping-pong groups) cover the column halves
    const int s = lane & 15, g = lane >> 4;
    const int grp = wave >> 2;
    const int ntiles = p.tiles_m * p.tiles_n;
    const int nk = p.K / R::BK;  // >= 8

    const int frag_row = (s >> 2) * 16 + (s & 3);
    const uint32_t chunk_off = (uint32_t)((g ^ (((s >> 2) & 1) * 3)) << 4);
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem;
    const uint32_t a_off = (uint32_t)((wm * 128 + frag_row) * R::ROWBYTES) + chunk_off;
    const uint32_t w_off = (uint32_t)((R::BM + wn * 64 + frag_row) * R::ROWBYTES) + chunk_off;
    const uint32_t slot_addr = lds_base + R::NST * R::STAGE;

    // LDS-DMA sources as 32-bit byte offsets from p.A / p.W (nt_v9_ok checks the range), of this tile and of the next one
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    u32x4_t src = {0, 0, 0, 0}, srcn = {0, 0, 0, 0};
    auto piece_offset = [&](int j, int m0, int n0) __attribute__((always_inline)) -> uint32_t {
        const int i = wave + 8 * j;
        const int row = R::ROWS_PER_PIECE * i + (lane >> R::CHUNK_SHIFT);
        const int slot = lane & (R::CHUNKS - 1);
        if (row < R::BM) {
            int m = m0 + row;
            if (m >= p.M) m = p.M - 1;
            return (uint32_t)(m * (int)p.lda + (slot ^ R::key(row)) * 8) * 2u;
        }
        const int wr = row - R::BM;
        return (uint32_t)((n0 + wr) * (int)p.ldw + (slot ^ R::key(wr)) * 8) * 2u;  // N % 256 == 0: every W row exists
    };
    auto issue = [&](bool of_next, int kslice, int stage) __attribute__((always_inline)) {
        const u32x4_t sv = of_next ? srcn : src;
#pragma unroll
        for (int j = 0; j < R::PIECES; ++j) {
            const int i = wave + 8 * j;
            const unsigned char* base = R::ROWS_PER_PIECE * i < R::BM ? p.A : p.W;  // wave-uniform: a piece is all A rows or all W rows
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + (sv[j] + (uint32_t)(kslice * R::BK * 2))),
                                             (__attribute__((address_space(3))) void*)(smem + stage * R::STAGE + i * 1024), 16, 0, 0);
        }
    };

    // ---- this workgroup's share of the tiles and its first draw (the protocol: common.hpp, beside sched_draw) ----
    const TileShare sh = tile_share(ntiles);
    const int xcnt = sh.cnt, xbase = sh.base, xgrid = sh.workers;
    const bool dyn = p.tile_slot >= 0;
    unsigned* const ctr = &g_tile_ctr[dyn ? p.tile_slot : 0][sh.part][0];
    bool reset_ctr = false;
    int pos = sh.index, m0, n0;
    if (dyn) {
        pos = sched_first_draw(ctr, slot_addr, wave);
        reset_ctr = sched_last_draw(sh, pos);
    }
    if (pos >= xcnt) {
        if (reset_ctr && tid == 0) sched_reset(ctr);
        return;
    }
    tile_origin<R::BM, R::BN>(xbase + pos, p.tiles_n, m0, n0);
#pragma unroll
    for (int j = 0; j < R::PIECES; ++j) src[j] = piece_offset(j, m0, n0);
    issue(false, 0, 0);
    issue(false, 1, 1);
    issue(false, 2, 2);
    int ring = 0;  // LDS stage of the current K slice; runs on across tiles
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * R::PIECES) : "memory");  // slice 0 landed
    __builtin_amdgcn_s_barrier();
    if (grp) __builtin_amdgcn_s_barrier();  // ping-pong: waves 4-7 run one barrier interval behind waves 0-3
    bool stores_behind = false;  // the previous tile's epilogue stores (exactly NSTORE per lane) are the youngest operations before this tile

    while (true) {
        int next = pos + xgrid;
        bool has_next = !dyn && next < xcnt;
        int nm0 = 0, nn0 = 0;
        uint32_t fetched = 0, seen = 0;
        f32x4_t acc0[4][4], acc1[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc0[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                acc1[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
        // One K iteration.  EX = how many of the previous tile's stores may still be in flight behind the slice this iteration waits
        // for (NSTORE in iterations 0 and 1 of a tile that follows a full tile, else 0); FX: 1 draw, 2 publish, 3 read (as v7).
        auto kstep = [&](int kt, auto EX, auto FX) __attribute__((always_inline)) {
            constexpr int ex = decltype(EX)::value, fx = decltype(FX)::value;
            const uint32_t stg = lds_base + ring * R::STAGE;
            uint4 wf[4], af0[4], af1[4];
            lds_read4<R::ROWBYTES>(wf, stg + w_off);
            lds_read4<R::ROWBYTES>(af0, stg + a_off);
            lds_read4<R::ROWBYTES>(af1, stg + a_off + 64 * R::ROWBYTES);
            if (fx == 3 && dyn) asm volatile("ds_read_b32 %0, %1" : "=v"(seen) : "v"(slot_addr) : "memory");
            const bool draw = fx == 1 && dyn && wave == 0;
            if (draw) sched_draw(fetched, ctr);
            asm volatile("" ::: "memory");
            const int stage3 = (ring + 3) & 3;
            // 0: nothing issued, 1: issued.  Slice kt + 3 of this tile, or slice kt + 3 - nk of the next one
            int issued = 1;
            if (kt + 3 < nk) issue(false, kt + 3, stage3);
            else if (has_next) issue(true, kt + 3 - nk, stage3);
            else issued = 0;
            const bool ext = ex > 0 && stores_behind;  // wave-uniform
#define V9_WAIT(n)                                                                   \
    do {                                                                             \
        if (draw) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((n) + 1) : "memory");     \
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory");                \
    } while (0)
            if (issued) {
                // slices kt + 2 and kt + 3 (2 x 4 pieces) stay in flight; in iterations 0 / 1 after a full tile the stores sit between
                // slice kt + 2 (issued before them) and slice kt + 3 (just issued): they may stay too
                if (ext) V9_WAIT(2 * R::PIECES + ex);
                else V9_WAIT(2 * R::PIECES);
            } else {
                // the last tile's last three iterations: slices kt + 1, kt + 2 may be all that is left -- keep it simple
                if (kt + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(R::PIECES) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
#undef V9_WAIT
            if (fx == 2 && dyn && wave == 0) sched_publish(slot_addr, fetched);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
            mfma_4x4<T>(acc0, wf, af0);
            mfma_4x4<T>(acc1, wf, af1);
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            ring = (ring + 1) & 3;
        };
        // (the barrier that closes an iteration is outside kstep: the very last one of a workgroup is skipped by waves 4-7, which made
        // one more at the start)
        // The draw of iteration 0 is YOUNGER than the previous tile's stores, which iterations 0 and 1 let stay in flight: only iteration
        // 2's wait (everything but the two youngest slices) retires it -> publish there, read in iteration 3.
        kstep(0, IC<NSTORE>(), IC<1>());
        __builtin_amdgcn_s_barrier();
        kstep(1, IC<NSTORE>(), IC<0>());
        __builtin_amdgcn_s_barrier();
        kstep(2, IC<0>(), IC<2>());
        __builtin_amdgcn_s_barrier();
        kstep(3, IC<0>(), IC<3>());
        __builtin_amdgcn_s_barrier();
        if (dyn) {
            next = __builtin_amdgcn_readfirstlane((int)seen);
            has_next = next < xcnt;
            reset_ctr = reset_ctr || sched_last_draw(sh, next);
        }
        if (has_next) {
            tile_origin<R::BM, R::BN>(xbase + next, p.tiles_n, nm0, nn0);
#pragma unroll
            for (int j = 0; j < R::PIECES; ++j) srcn[j] = piece_offset(j, nm0, nn0);
        }
        for (int kt = 4; kt < nk; ++kt) {
            kstep(kt, IC<0>(), IC<0>());
            if (!(grp && kt + 1 == nk && !has_next)) __builtin_amdgcn_s_barrier();
        }
        // ---- epilogue: the one-shot kernels' (its loads wait for the counter to drain, i.e. also for the next tile's three slices --
        // which the next K loop needs at once anyway); its stores stay in flight into the next tile ----
        gemm_epilogue_fast<T, OUT_F32, F>(p, acc0, m0 + wm * 128, n0 + wn * 64, lane);
        gemm_epilogue_fast<T, OUT_F32, F>(p, acc1, m0 + wm * 128 + 64, n0 + wn * 64, lane);
        if (!has_next) break;
        const bool full = m0 + R::BM <= p.M;
        if (!full) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // rows beyond M: fewer stores than NSTORE were issued, count nothing
        stores_behind = full;
        asm volatile("" ::: "memory");
        pos = next;
        m0 = nm0;
        n0 = nn0;
        src = srcn;
    }
    if (reset_ctr && tid == 0) sched_reset(ctr);
}

bool nt_v9_ok(const GemmP& p, int f, bool out_f32) {
    typedef WideRing R;
    if (p.a_mode == LNX_ADDR_PATCH2) return false;
    if (p.N % R::BN != 0 || p.K % R::BK != 0 || p.K / R::BK < 8) return false;
    return fits_32bit_offsets(p) && nt_v4_carries(out_f32, f);
}

int launch_nt_v9(const GemmP& p0, int f, bool out_f32, hipStream_t st) {
    typedef WideRing R;
    GemmP p = p0;
    p.tiles_m = cdiv(p.M, R::BM);
    p.tiles_n = p.N / R::BN;
    size_t lds;
    const int grid = persistent_geometry<R>(p, st, lds);
    LNX_CHECK(grid > 0, "gemm_nt_v9: no device");
    return with_nt_form<nt_v4_carries>("gemm_nt_v9", out_f32, f, [&](auto form) {
        using Form = decltype(form);
        return launch_with_lds<gemm_nt_v9_kernel<Form::out_f32, Form::f>>(grid, 512, lds, st, p);
    });
}

}  // namespace lnxg
