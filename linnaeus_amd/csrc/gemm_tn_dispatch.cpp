// The TN (weight-gradient) GEMM dispatch: which kernel lnx_gemm_tn gives a product, in which tile form, how the contraction is split and
// whether the partial tiles meet in the workspace (tn_plan), and the two entry points that rest on it -- lnx_gemm_tn_query answers
// without a launch or a GPU, lnx_gemm_tn launches.  Host code only; the kernels and their launchers are in gemm.hip (128x128) and
// gemm2.hip (LDS-DMA ring, second stages).
#include <stdlib.h>

#include "gemm_common.hpp"

namespace lnxg {

bool tn_v2_ok(const WgradP& p, int dtype) {
    return dtype == LNX_BF16 && p.M % TN_RING_ROWS == 0 && p.M >= 4096 && p.N >= 8 && p.K >= 8;
}

TnPlan tn_plan(const WgradP& p, int dtype, int splits_hint) {
    TnPlan t{};
    t.patch = p.a_mode == LNX_ADDR_PATCH2;
    t.ring = tn_v2_ok(p, dtype) && !nt_switches().force_v1;
    if (!t.ring) {
        t.RW = t.CW = TILE;
        t.tiles_n = cdiv(p.N, TILE);
        t.tiles_k = cdiv(p.K, TILE);
        const int bmc = dtype == LNX_BF16 ? 64 : 32;
        int splits = splits_hint;
        if (splits <= 0) {
            // aim at ~2 workgroups per CU, but keep >= 4 M-tiles of work per split
            const int tiles = t.tiles_n * t.tiles_k;
            splits = cdiv(2 * 256, tiles);
            const int max_splits = cdiv(p.M, 4 * bmc);
            if (splits > max_splits) splits = max_splits;
            if (splits < 1) splits = 1;
        }
        // deterministic mode: this kernel has no workspace second stage, its splits meet in float atomics -- one split, one contributor
        // per element
        if (deterministic()) splits = 1;
        int mps = cdiv(p.M, splits);
        mps = cdiv(mps, bmc) * bmc;
        t.splits = cdiv(p.M, mps);
        t.m_per_split = mps;
        t.workspace = false;
        return t;
    }
    // tile orientation with the least padding waste
    auto waste = [&](int rw, int cw) { return (double)cdiv(p.N, rw) * rw * cdiv(p.K, cw) * cw; };
    static const char* force = getenv("LNX_TN_ORIENT");  // A/B switch: "r" = 256x128 tiles, "c" = 128x256
    const bool wide_r = force ? force[0] == 'r' : waste(256, 128) <= waste(128, 256);
    const int RW = wide_r ? 256 : 128, CW = wide_r ? 128 : 256;
    t.RW = RW;
    t.CW = CW;
    t.tiles_n = cdiv(p.N, RW);
    t.tiles_k = cdiv(p.K, CW);
    const int tiles = t.tiles_n * t.tiles_k;
    const int mtiles = p.M / TN_RING_ROWS;
    int splits = splits_hint;
    if (splits <= 0) {
        splits = 256 / tiles;  // the 144 KiB ring allows one workgroup per CU: at most one full round
        if (splits < 1) splits = 1;
        const int max_splits = mtiles / 8 > 0 ? mtiles / 8 : 1;  // ... with >= 8 contraction tiles each
        if (splits > max_splits) splits = max_splits;
    }
    if (splits > mtiles) splits = mtiles;
    if (splits < 1) splits = 1;
    const bool det = deterministic();
    auto ws_need = [&](int sp) { return (size_t)sp * tiles * (256 * 128) + (size_t)sp * t.tiles_n * RW; };
    const size_t have = p.ws ? (size_t)p.ws_floats : 0;
    if (det) {
        // deterministic mode: two or more splits always meet in the workspace second stage (fixed order); where the workspace cannot
        // hold them the contraction is split less, down to one workgroup per output tile (one contributor per element)
        while (splits > 1 && ws_need(cdiv(mtiles, cdiv(mtiles, splits))) > have) --splits;
    }
    const int per = cdiv(mtiles, splits);
    t.m_per_split = per * TN_RING_ROWS;
    t.splits = cdiv(mtiles, per);
    static const bool no_ws = getenv("LNX_TN_ATOMIC") != nullptr;  // A/B switch for benchmarking
    // padded tiles are stored and re-read whole: with poorly filled tiles (N x K well below tiles x 256 x 128) the atomics move fewer bytes
    const bool sparse_tiles = (double)p.N * p.k_store < 0.7 * (double)tiles * (256 * 128);
    if (det) t.workspace = t.splits >= 2;  // (the loop above made the workspace fit)
    else t.workspace = !(no_ws || p.ws == nullptr || have < ws_need(t.splits) || t.splits < 2 || sparse_tiles);
    return t;
}

}  // namespace lnxg

namespace {

// what the decision looks at, checked the same way for the launch and the query (1 and lnx_last_error on a bad problem)
int tn_check_sizes(const lnx_wgrad_args* a, const char* who) {
    LNX_CHECK(a != nullptr, "%s: null args", who);
    LNX_CHECK(a->dtype == LNX_F32 || a->dtype == LNX_BF16, "%s: bad dtype %d", who, a->dtype);
    const int epv = a->dtype == LNX_F32 ? 4 : 8;
    LNX_CHECK(a->M > 0 && a->N > 0 && a->K > 0, "%s: empty problem", who);
    // dY rows are read in 16-byte chunks: a chunk that starts below N may run past it, so the row
    // must be padded (lddy >= roundup(N, epv)); what the padding holds is never stored
    LNX_CHECK(a->lddy % epv == 0 && a->lddy >= (int64_t)cdiv(a->N, epv) * epv, "%s: lddy=%lld must be a multiple of %d and >= roundup(N)", who, (long long)a->lddy, epv);
    LNX_CHECK(a->K % epv == 0, "%s: K=%d must be a multiple of %d", who, a->K, epv);
    if (a->a_mode == LNX_ADDR_PATCH2) {
        LNX_CHECK(a->Hin % 2 == 0 && a->Win % 2 == 0 && a->Cin % epv == 0 && a->K == 4 * a->Cin, "%s: bad PATCH2 geometry", who);
    } else {
        LNX_CHECK(a->lda % epv == 0, "%s: lda must be a multiple of %d", who, epv);
    }
    if (a->k_perm_c > 0) LNX_CHECK(a->K % a->k_perm_c == 0, "%s: K %% k_perm_c != 0", who);
    return 0;
}

// the one place a lnx_wgrad_args becomes a WgradP (tiles, splits and the workspace decision come from tn_plan afterwards)
void fill_wgrad_p(const lnx_wgrad_args* a, WgradP& p) {
    p.dY = (const unsigned char*)a->dY;
    p.A = (const unsigned char*)a->A;
    p.dW = a->dW;
    p.db = a->db;
    p.lddy = a->lddy;
    p.lda = a->lda;
    p.lddw = a->lddw;
    p.M = a->M;
    p.N = a->N;
    p.K = a->K;
    p.a_mode = a->a_mode;
    p.pg = PatchGeom{a->Hin, a->Win, a->Cin};
    p.k_perm_c = a->k_perm_c;
    p.ws = a->ws;
    p.ws_floats = a->ws ? a->ws_floats : 0;
    p.k_store = (a->k_store > 0 && a->k_store < a->K) ? a->k_store : a->K;
    p.m_dev = a->m_dev;
}

}  // namespace

// The decision without a launch (include/lnx.h): sizes, dtype, modes and WHICH of ws / db are present -- no pointer is dereferenced.
extern "C" int lnx_gemm_tn_query(const lnx_wgrad_args* a, lnx_tn_launch* out) {
    LNX_CHECK(out != nullptr, "lnx_gemm_tn_query: null result");
    if (tn_check_sizes(a, "lnx_gemm_tn_query") != 0) return 1;
    WgradP p;
    fill_wgrad_p(a, p);
    const TnPlan t = tn_plan(p, a->dtype, a->splits);
    out->kernel = t.ring ? LNX_TN_KERNEL_RING : LNX_TN_KERNEL_V1;
    out->rw = t.RW;
    out->cw = t.CW;
    out->patch = t.patch ? 1 : 0;
    out->tiles_n = t.tiles_n;
    out->tiles_k = t.tiles_k;
    out->splits = t.splits;
    out->m_per_split = t.m_per_split;
    out->workspace = t.workspace ? 1 : 0;
    return 0;
}

extern "C" int lnx_gemm_tn(const lnx_wgrad_args* a, void* stream) {
    if (tn_check_sizes(a, "lnx_gemm_tn") != 0) return 1;
    LNX_CHECK(a->dY && a->A && a->dW, "lnx_gemm_tn: null operand");
    LNX_CHECK((((uintptr_t)a->A) & 15) == 0 && (((uintptr_t)a->dY) & 15) == 0, "lnx_gemm_tn: operands must be 16-byte aligned");
    WgradP p;
    fill_wgrad_p(a, p);
    const TnPlan t = tn_plan(p, a->dtype, a->splits);
    p.tiles_n = t.tiles_n;
    p.tiles_k = t.tiles_k;
    p.splits = t.splits;
    p.m_per_split = t.m_per_split;
    if (t.ring && !t.workspace) p.ws = nullptr;  // (the ring kernel takes ws != nullptr for "store the partial tiles")
    hipStream_t st = (hipStream_t)stream;
    static const bool no_defer = getenv("LNX_TN_NO_DEFER") != nullptr;  // A/B switch: every product reduces its own partial tiles at once
    int rc;
    if (t.ring) rc = launch_tn_v2(p, t, st, a->defer != 0 && !no_defer);
    else rc = launch_tn_v1(p, a->dtype, st);
    if (rc != 0) return rc;
    LNX_LAUNCH_CHECK();
    return 0;
}
