// The NT GEMM dispatch: which kernel family lnx_gemm_nt gives a product (nt_choose), the A/B switches that bend the choice
// (nt_switches), and the two entry points that rest on it -- lnx_nt_dispatch answers without a launch or a GPU, lnx_gemm_nt launches.
// Host code only; the kernels and their launchers are in gemm.hip (v1), gemm_skinny.hip, gemm2.hip (v2, v4), gemm3.hip (v7),
// gemm5.hip (v9) and gemm_fp8.hip (fp8 / mx8: entry points of their own, same switches and bookkeeping).
#include <stdlib.h>

#include <atomic>

#include "gemm_common.hpp"

// dispatch bookkeeping (include/lnx.h: lnx_last_nt_kernel / lnx_nt_kernel_launches)
static std::atomic<int> g_last_nt{0};
static std::atomic<long long> g_nt_launches[LNX_NT_KERNEL_KINDS];
extern "C" int lnx_last_nt_kernel(void) { return g_last_nt.load(std::memory_order_relaxed); }
extern "C" int64_t lnx_nt_kernel_launches(int kind) {
    return (kind < 0 || kind >= LNX_NT_KERNEL_KINDS) ? -1 : (int64_t)g_nt_launches[kind].load(std::memory_order_relaxed);
}

namespace lnxg {

void note_nt_kernel(int kind) {
    if (kind < 0 || kind >= LNX_NT_KERNEL_KINDS) return;
    g_last_nt.store(kind, std::memory_order_relaxed);
    g_nt_launches[kind].fetch_add(1, std::memory_order_relaxed);
}

nt_experiment_fn g_nt_experiment = nullptr;

int nt_form_error(const char* family, bool out_f32, int f) {
    lnx_set_error("%s: no kernel is compiled for the epilogue form f = %d with %s output", family, f, out_f32 ? "an fp32" : "a storage-type");
    return 1;
}

static int env_int(const char* name, int unset) {
    const char* e = getenv(name);
    return e ? atoi(e) : unset;
}

NtSwitches nt_switches() {
    static const NtSwitches latched = [] {
        NtSwitches s{};
        s.force_v1 = getenv("LNX_GEMM_V1") != nullptr;  // A/B switch for benchmarking
        s.skinny = env_int("LNX_NT_SKINNY", 1) != 0;
        s.v4 = env_int("LNX_NT_V4", 1) != 0;  // A/B switch for benchmarking
        s.tile_cost = env_int("LNX_NT_TILE_COST", 1) != 0;
        s.generic_epi = getenv("LNX_NT_GENERIC_EPI") != nullptr;  // A/B switch for benchmarking
        return s;
    }();
    NtSwitches s = latched;
    s.v7 = env_int("LNX_NT_V7", -1);
    s.v9 = env_int("LNX_NT_V9", -1);
    s.fp8_x8 = env_int("LNX_FP8_X8", 1) != 0;
    return s;
}

void fill_gemm_p(const lnx_gemm_args* a, GemmP& p) {
    p.A = (const unsigned char*)a->A;
    p.W = (const unsigned char*)a->W;
    p.C = (unsigned char*)a->C;
    p.C2 = (unsigned char*)a->c2;
    p.aux = (const unsigned char*)a->aux;
    p.bias = a->bias;
    p.gamma = a->gamma;
    p.rowscale = a->rowscale;
    p.res = a->res;
    p.lda = a->lda;
    p.ldw = a->ldw;
    p.ldc = a->ldc;
    p.ldc2 = a->ldc2;
    p.ldaux = a->ldaux;
    p.ldres = a->ldres;
    p.M = a->M;
    p.M_host = a->M;
    p.m_dev = a->m_dev;
    p.perm = a->perm;
    p.N = a->N;
    p.K = a->K;
    p.a_mode = a->a_mode;
    p.c_mode = a->c_mode;
    p.pg = PatchGeom{a->Hin, a->Win, a->Cin};
    p.cmap = RowMap{a->c_map.group, a->c_map.pad, a->c_map.off};
    p.act = a->act;
    p.rows_per_sample = a->rows_per_sample > 0 ? a->rows_per_sample : 1;
    p.tiles_m = cdiv(a->M, TILE);
    p.tiles_n = cdiv(a->N, TILE);
}

// default choice (LNX_NT_V7 unset): from the measurements of tools/bench_gemm_epi.py
// Measured (profiles/r03_nt_v7.log, sm shapes at B = 256): against the one-shot 256x128 kernel the persistent kernel wins
// 10-30 % when it has at least two tiles per CU (no pipeline refill per tile, stores spread over the K loop) and the epilogue is
// light (plain / bias / fp32 residual); it ties with the 256x256 kernel where that one applies (N % 256 == 0) and with the GELU
// forms (their epilogue arithmetic, not their stores, is what the K loop waits for), and loses a few percent below two tiles
// per CU.
// Round 4: 256x256 or 256x128 tiles for a product whose N allows both?  Every tile of a launch costs the same, so a launch takes
// ceil(tiles / CUs) rounds whatever the scheduler: 600 tiles of 256x256 on 256 CUs are three rounds for 2.3 rounds of work (the
// N = 1536 products of BASELINE config 3's 128 images per GPU), the same product in 1200 tiles of 256x128 five half-size rounds.  The
// big tile moves 1.5x fewer operand bytes per FLOP, which is worth ~3 % at K = 384 and ~12 % on long K loops (profiles/r03_bare_gemm.log).
// LNX_NT_TILE_COST=0: the round-3 rule (big tile wherever N % 256 == 0).
static bool big_tile_wins(const GemmP& p, const NtSwitches& sw) {
    if (!sw.tile_cost) return true;
    const int dc = device_cus();
    const int cus = persistent_cus(dc > 0 ? dc : 256);
    const int64_t rows = cdiv(p.M, 256);
    const double big = (double)cdiv(rows * (p.N / WideRing::BN), (int64_t)cus) * 2.0 * (p.K <= 512 ? 0.97 : 0.88);
    const double small = (double)cdiv(rows * cdiv(p.N, 128), (int64_t)cus);
    return small >= 0.93 * big;  // (the small tile has to win by a margin: measured, a tie on paper goes to the big tile at sm / lg / xl)
}

static bool nt_v7_preferred(const GemmP& p, int f, bool out_f32, const NtSwitches& sw) {
    const bool two_per_cu = (int64_t)cdiv(p.M, 256) * cdiv(p.N, 128) >= 512;
    const bool big_better = p.N % WideRing::BN == 0 && big_tile_wins(p, sw);
    if (f == F_GELU_BWD && p.act == LNX_ACT_MUL_AUX) return two_per_cu;  // 121.6 -> 115.7 us at the sm fc2 data gradient, also against the 256x256 tile
    if (f == F_GELU_BWD || f == (F_BIAS | F_C2 | F_GELU)) return two_per_cu && p.N % WideRing::BN == 0 && !big_better;  // only instead of a badly filling big tile
    if (f != 0 && f != F_BIAS && !(out_f32 && f == (F_BIAS | F_RES))) return false;
    if (big_better) return false;  // the 256x256 tile (half the fill traffic per FLOP) is the better kernel there
    return two_per_cu;
}

static bool nt_v4_ok(const GemmP& p, int f, const NtSwitches& sw) {
    if (!sw.v4 || f == (int)F_GENERIC || p.a_mode == LNX_ADDR_PATCH2) return false;
    return p.N % WideRing::BN == 0 && p.K % WideRing::BK == 0 && p.K >= 4 * WideRing::BK;
}

static bool nt_v2_ok(const GemmP& p, int dtype) {
    if (dtype != LNX_BF16) return false;
    if (p.K % 64 != 0 || p.K < 128) return false;
    if (p.M < 1024) return false;  // tiny-M GEMMs (tail, meta heads) stay on the 128x128 kernel
    return true;
}

// The whole decision, in order: skinny -> the 128x128 kernel for what the pipelined kernels cannot run (or LNX_GEMM_V1) -> the epilogue
// mask -> persistent 256x128 -> 256x256, persistent or one-shot -> one-shot 256x128.  These are the rules of DESIGN.md's dispatch table:
//   LNX_NT_V7: 1 = every shape the persistent deferred-store kernel can run, 0 = never, unset = the measured choice (nt_v7_preferred)
//   LNX_NT_V9: 1 = the persistent 256x256 kernel wherever it can run, 0 = never, unset = with at least 1.5 tiles per CU (below that a
//              workgroup has no second tile to hide the first one's epilogue under) and where the big tile wins on rounds
NtChoice nt_choose(const GemmP& p, int dtype, bool out_f32) {
    const NtSwitches sw = nt_switches();
    // (compact rows -- m_dev / perm -- are carried by every family but the skinny kernel, whose M <= 256 products then go to the 128x128 one)
    if (sw.skinny && !sw.force_v1 && !p.m_dev && !p.perm && nt_skinny_ok(p, dtype, out_f32)) return {LNX_NT_KERNEL_SKINNY, 0};
    if (sw.force_v1 || !nt_v2_ok(p, dtype)) return {LNX_NT_KERNEL_V1, 0};
    const int f = (p.a_mode == LNX_ADDR_PATCH2 || sw.generic_epi) ? (int)F_GENERIC : fast_epilogue_mask(p, out_f32);
    if (sw.v7 != 0 && nt_v7_ok(p, f, out_f32) && (sw.v7 == 1 || nt_v7_preferred(p, f, out_f32, sw))) return {LNX_NT_KERNEL_V7, f};
    if (nt_v4_ok(p, f, sw) && (sw.v9 == 1 || big_tile_wins(p, sw))) {
        const int dc = device_cus();
        const int64_t cus = dc > 0 ? dc : 256;
        if (sw.v9 != 0 && nt_v9_ok(p, f, out_f32) && (sw.v9 == 1 || (int64_t)cdiv(p.M, WideRing::BM) * (p.N / WideRing::BN) * 2 >= 3 * cus)) return {LNX_NT_KERNEL_V9, f};
        return {LNX_NT_KERNEL_V4, f};
    }
    return {LNX_NT_KERNEL_V2, f};
}

}  // namespace lnxg

// The dispatcher's decision without a launch (include/lnx.h): only M / N / K / dtype / out_f32 / act / addressing modes and WHICH of the
// optional operands are present matter -- the pointers are never dereferenced, so a host-side caller may pass any non-null value.
extern "C" int lnx_nt_dispatch(const lnx_gemm_args* a) {
    if (!a || a->M <= 0 || a->N <= 0 || a->K <= 0 || (a->dtype != LNX_F32 && a->dtype != LNX_BF16)) return -1;
    GemmP p;
    fill_gemm_p(a, p);
    return nt_choose(p, a->dtype, a->out_f32 != 0).kind;
}

extern "C" int lnx_gemm_nt(const lnx_gemm_args* a, void* stream) {
    LNX_CHECK(a != nullptr, "lnx_gemm_nt: null args");
    LNX_CHECK(a->dtype == LNX_F32 || a->dtype == LNX_BF16, "lnx_gemm_nt: bad dtype %d", a->dtype);
    const int epv = a->dtype == LNX_F32 ? 4 : 8;
    LNX_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "lnx_gemm_nt: empty problem M=%d N=%d K=%d", a->M, a->N, a->K);
    LNX_CHECK(a->K % epv == 0, "lnx_gemm_nt: K=%d must be a multiple of %d", a->K, epv);
    LNX_CHECK(a->A && a->W && a->C, "lnx_gemm_nt: null operand");
    LNX_CHECK(a->ldw % epv == 0, "lnx_gemm_nt: ldw=%lld must be a multiple of %d", (long long)a->ldw, epv);
    LNX_CHECK((((uintptr_t)a->A) & 15) == 0 && (((uintptr_t)a->W) & 15) == 0, "lnx_gemm_nt: A/W must be 16-byte aligned");
    if (a->a_mode == LNX_ADDR_PATCH2) {
        LNX_CHECK(a->Hin % 2 == 0 && a->Win % 2 == 0 && a->Cin % epv == 0, "lnx_gemm_nt: bad PATCH2 geometry %dx%dx%d", a->Hin, a->Win, a->Cin);
        LNX_CHECK(a->K == 4 * a->Cin, "lnx_gemm_nt: PATCH2 needs K == 4*Cin");
        LNX_CHECK(a->M % ((a->Hin / 2) * (a->Win / 2)) == 0, "lnx_gemm_nt: PATCH2 needs M == B*Ho*Wo");
    } else {
        LNX_CHECK(a->lda % epv == 0, "lnx_gemm_nt: lda=%lld must be a multiple of %d", (long long)a->lda, epv);
    }
    if (a->c_mode == LNX_ADDR_PATCH2) {
        LNX_CHECK(a->Hin % 2 == 0 && a->Win % 2 == 0 && a->Cin % 16 == 0, "lnx_gemm_nt: bad PATCH2 output geometry");
        LNX_CHECK(a->N == 4 * a->Cin, "lnx_gemm_nt: PATCH2 output needs N == 4*Cin");
        LNX_CHECK(a->a_mode == LNX_ADDR_PLAIN, "lnx_gemm_nt: PATCH2 on both sides is not supported");
    }
    LNX_CHECK(a->act >= LNX_ACT_NONE && a->act <= LNX_ACT_MUL_AUX, "lnx_gemm_nt: unknown act %d", a->act);
    if (a->act == LNX_ACT_GELU_BWD || a->act == LNX_ACT_RELU_BWD || a->act == LNX_ACT_MUL_AUX) LNX_CHECK(a->aux != nullptr, "lnx_gemm_nt: act %d needs aux", a->act);
    if (a->act == LNX_ACT_GELU_D) LNX_CHECK(a->c2 != nullptr, "lnx_gemm_nt: GELU_D writes the derivative to c2, which is NULL");
    if (a->rowscale) LNX_CHECK(a->rows_per_sample > 0, "lnx_gemm_nt: rowscale needs rows_per_sample");
    if (a->perm) {
        LNX_CHECK(a->rows_per_sample > 0 && a->M % a->rows_per_sample == 0 && a->c_mode == LNX_ADDR_PLAIN && a->c_map.group == 0 && a->c_map.off == 0,
                  "lnx_gemm_nt: perm needs rows_per_sample, M a whole number of samples and plain C addressing with an identity row map");
        // (the fast epilogues translate rows where they look the row scale up, and only their residual form does)
        LNX_CHECK(a->res && a->rowscale, "lnx_gemm_nt: perm is for the residual form with a row scale (it needs res and rowscale)");
    }

    GemmP p;
    fill_gemm_p(a, p);
    const bool out_f32 = a->out_f32 != 0;
    hipStream_t st = (hipStream_t)stream;
    const NtChoice c = nt_choose(p, a->dtype, out_f32);
    const bool pipelined = c.kind == LNX_NT_KERNEL_V2 || c.kind == LNX_NT_KERNEL_V4 || c.kind == LNX_NT_KERNEL_V7 || c.kind == LNX_NT_KERNEL_V9;
    // measurement kernels kept outside the product (tools/experiments/: gemm_nt_v5, gemm_nt_v8) hook in here, in front of every pipelined
    // launch, when their library is the one loaded (LNX_LIB_PATH=tools/liblnx_experiments.so); the shipped library never sets the hook
    if (pipelined && g_nt_experiment && g_nt_experiment(p, c.f, out_f32, st) == 0) {
        LNX_LAUNCH_CHECK();
        return 0;
    }
    note_nt_kernel(c.kind);
    int rc = 1;
    switch (c.kind) {
        case LNX_NT_KERNEL_SKINNY: rc = launch_nt_skinny(p, out_f32, st); break;
        case LNX_NT_KERNEL_V1: rc = launch_nt_v1(p, a->dtype, out_f32, st); break;
        case LNX_NT_KERNEL_V2: rc = launch_nt_v2(p, c.f, out_f32, st); break;
        case LNX_NT_KERNEL_V4: rc = launch_nt_v4(p, c.f, out_f32, st); break;
        case LNX_NT_KERNEL_V7: rc = launch_nt_v7(p, c.f, out_f32, st); break;
        case LNX_NT_KERNEL_V9: rc = launch_nt_v9(p, c.f, out_f32, st); break;
        default: lnx_set_error("lnx_gemm_nt: the dispatcher chose kernel family %d, which has no launcher here", c.kind);
    }
    if (rc != 0) return rc;
    LNX_LAUNCH_CHECK();
    return 0;
}
