// mFormerV1 forward/backward plan: the native runtime of the path.
//
// One lnx_plan_forward / lnx_plan_backward call enqueues every kernel of a training step's
// model work on the caller's HIP stream (no allocation, no host sync, no Python between
// kernels).  Orchestration follows mFormerV1.forward_features (models/mFormerV1.py:407-529),
// restated for NHWC / token-major buffers:
//
//   activations      T (bf16 | fp32) row-major [rows, channels]; conv stages are NHWC
//   residual stream  fp32 (what autocast keeps in fp32 in the reference)
//   parameters/grads fp32, caller-owned; a T-typed operand arena is refreshed every forward
//   saved-for-backward tensors live in the workspace until the next forward
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/lnx.h"

void lnx_set_error(const char* fmt, ...);

#define RUN(expr)                  \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_ != 0) return rc_;  \
    } while (0)
#define FAIL(...)                   \
    do {                            \
        lnx_set_error(__VA_ARGS__); \
        return 1;                   \
    } while (0)
#define HIPRUN(expr)                                                         \
    do {                                                                     \
        const hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) FAIL("%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace {

constexpr int LN_DEFER_SLOTS = 16;  // == norm.hip's LN_BATCH: postponed LayerNorm-backward reductions per flush
constexpr int FREQ_DEFER_SLOTS = 8;  // <= LNX_ATTN_DEFER_MAX: attention backward calls whose freqs fold waits for the segment's flush

inline int64_t align_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }

struct OpW {          // a GEMM weight in the T-typed operand arena
    int param = -1;   // source parameter
    int N = 0, K = 0; // logical [N, K]
    int ld = 0;       // leading dimension of the [N, ld] copy (K zero-padded)
    int ld_t = 0;     // leading dimension of the transposed [K, ld_t] copy (0: none)
    int mode = LNX_PREP_CAST, P = 0;
    bool f32 = false;  // operand kept in fp32 even in bf16 mode (the tiny M = batch meta-head GEMMs)
    int64_t off = 0, off_t = 0;
    int64_t off8 = 0, off8s = 0;  // fp8 plans: MXFP8 copy [N][K] bytes and its block scales [K/128][N][4] (0: none)
    int64_t off8t = 0, off8ts = 0;  // ... and of the transposed weight [K][N] (data-gradient products), scales [N/128][K][4]
};

struct ConvBlk {
    bool fused = false;  // pwconv1 -> GELU -> pwconv2 -> LayerScale -> residual in one kernel (hidden tensor stays on chip)
    bool fused_ln = false;  // ... and the block LayerNorm (forward and backward) inside those kernels: no separate LayerNorm pass
    int gamma, dww, dwb, lnw, lnb, b1, b2;
    OpW w1, w2;
    int64_t w49;  // fp32 [49][C] in the arena
    // saved
    // hpre, act, z: unfused blocks only.  A fused block keeps the hidden tensor on chip and reads its LayerScale gradient off the pwconv2
    // weight gradient (lnx_layerscale_apply_wgrad), so z is neither written nor read
    int64_t xin, y, ln, mean, rstd, hpre, act, z;
};
struct RopeBlk {
    int n1w, n1b, n2w, n2b, freqs, qkvb, projb, fc1b, fc2b;
    OpW qkv, proj, fc1, fc2;
    int64_t xin, n1, mean1, rstd1, qkvbuf, cos, dsin, o, lse, xmid, n2, mean2, rstd2, hpre, act;
    int64_t dm_proj = 0, dm_hid = 0, dm_fc2 = 0;  // byte offsets of this block's dropout keep masks in the caller's mask buffer
    int64_t dm_attn = 0;                          // ... and of its attention-probability keep mask in the second buffer
};
struct MetaHead {
    int b0, lnw0, lnb0, nf1w, nf1b, nf2w, nf2b, b1, b2;
    OpW w0, w1, w2;
    int dim, off;
    int64_t t0, h0, x, m0, r0, h1, n1, m1, r1, h2, m2, r2;
    int64_t dp2 = 0, dp1 = 0, dp0 = 0, part = 0;  // one-launch chain (metahead.hip): backward scratch of this head
};
struct Down {
    int lnw, lnb, cb;
    OpW w;
    int64_t ln, mean, rstd;
};

}  // namespace

constexpr int TN_WS_SLOTS = 4;  // split-K workspace regions: the weight-gradient products of one block reduce in one launch

struct lnx_plan {
    lnx_mformer_cfg c;
    int esz;  // sizeof(T)
    int E;    // extra tokens
    int H[4], W[4], HW[4];
    int Ntok[2];  // tokens per sample of the two RoPE stages: HW + E
    std::vector<std::string> names;
    std::vector<int64_t> numel;
    std::vector<signed char> seg;  // the backward segment (0-3) after which the parameter's gradient is final
    // Units: the model in forward order -- stem, conv blocks, downsample 1, conv blocks, downsample 2, tokens_1, RoPE blocks, mid,
    // tokens_2, RoPE blocks, tail, heads.  `cut` is the first unit that holds a trainable parameter (lnx_plan_set_trainable; 0 = everything
    // trains): the units before it run forward-only on shared activation buffers and the backward stops behind unit `cut`.
    std::vector<std::string> unit_names;
    std::vector<int> unit_of;  // unit of each parameter
    int u_conv[2] = {0, 0}, u_down[2] = {0, 0}, u_tok[2] = {0, 0}, u_rope[2] = {0, 0}, u_mid = 0, u_tail = 0, u_heads = 0;
    int cut = 0;
    bool frozen_prefix = true;  // LNX_FROZEN_PREFIX=0 (read at creation): lnx_plan_set_trainable accepts and ignores its mask (A/B switch)
    int bwd_units = 0;          // units the last backward ran (lnx_plan_last_backward_units)
    bool runs(int unit) const { return unit >= cut; }  // the backward runs this unit
    // Input gradients (lnx_plan_set_input_grads): the backward's data path continues to the image (want_x: the cut is the stem) / to the
    // metadata (want_meta: the cut is tokens_1 at the latest) whatever the mask says; mask_cut keeps what lnx_plan_set_trainable asked for
    // (the number of units: an all-zero mask, legal only with a flag set).  dx_out / dmeta_out: where the next backward writes them
    // (lnx_plan_bind_input_grads; NULL = not this time); hold_input_grads: lnx_plan_backward_into is running, which never writes them.
    int mask_cut = 0;
    bool want_x = false, want_meta = false, hold_input_grads = false;
    float *dx_out = nullptr, *dmeta_out = nullptr;
    int64_t o_dcol = 0;  // want_x without lnx_stem_dgrad: the [M0, in_chans * 16] product between lnx_gemm_nt and lnx_col2im_stem
    float* dmeta_dst() const { return want_meta && !hold_input_grads ? dmeta_out : nullptr; }
    std::vector<const float*> P;
    std::vector<float*> G;
    bool bound = false, has_grads = false, fwd_done = false;
    unsigned char* ws = nullptr;
    int64_t ws_bytes = 0;

    // parameters
    int stem_b, stem_lnw, stem_lnb, cls[2], norm_w[2], norm_b[2], fin_w, fin_b, agg_w, agg_b, cl_b1, cl_b2, cl_lnw, cl_lnb;
    OpW stem_w, cl_w1, cl_w2;
    std::vector<int> head_b;
    std::vector<OpW> head_w;
    std::vector<int> logit_ld;
    std::vector<int64_t> logit_off;
    int64_t logits_numel = 0;
    Down down[3];
    std::vector<ConvBlk> conv[2];
    std::vector<RopeBlk> rope[2];
    std::vector<MetaHead> meta[2];
    std::vector<OpW*> all_w;
    std::vector<int> drop_conv[2], drop_attn[2], drop_mlp[2];
    int n_drop = 0;

    // workspace offsets
    int64_t o_descs = 0, n_descs = 0, prep_blocks = 0;
    int64_t arena_end = 0;  // end of the weight copies: zeroed at bind, so that their K / N padding stays zero across refreshes
    int64_t n_descs_t = 0, n_descs_f = 0, prep_blocks_f = 0;  // T-typed table first, fp32-typed table after it
    int64_t o_patches, o_stem_pre, o_stem_mean, o_stem_rstd;
    int64_t o_stage_out[4];   // fp32 output of each stage (input of the next downsample / norm)
    int64_t o_tok[2];         // fp32 token buffers entering RoPE stages
    int64_t o_t1, o_t1_mean, o_t1_rstd;           // norm_1 output (T) + stats
    int64_t o_cl_hpre, o_cl_act, o_cl_u, o_cl_mean, o_cl_rstd, o_c1n;
    int64_t o_c2n, o_n2_mean, o_n2_rstd, o_agg, o_fin_mean, o_fin_rstd, o_feats, o_featsT;
    int64_t o_g[4];           // fp32 gradient streams per stage
    int64_t o_sA, o_sB = 0, o_sC, o_sD; // T scratch: [M,4C] / [M,4C] (fused conv-MLP backward) / [M,C] / [M,C]
    int64_t o_lnws = 0, lnws_floats = 0, o_lnws_side = 0, lnws_side_floats = 0;
    int64_t lnws_defer_floats = 0;
    int64_t o_lnws_defer = 0;  // LN_DEFER_SLOTS partial-sum regions of lnws_defer_floats each: LayerNorm backward calls whose second stage waits for the segment's flush
    int ln_pending = 0;        // ... how many of them are in use since the last flush
    int64_t gcos_floats = 0;   // floats of one freqs-gradient partial region (o_gcos holds FREQ_DEFER_SLOTS of them)
    int freq_pending = 0;      // attention backward calls whose freqs fold is postponed (lnx_attn_bwd_args.defer_freqs)
    bool freq_defer = true;    // LNX_FREQ_DEFER=0: fold inside every lnx_attn_bwd call (A/B switch)
    bool ln_defer = true;      // LNX_LN_DEFER=0: every LayerNorm backward reduces its column partials at once (A/B)
    int64_t o_tnws = 0;  // split-K workspace of the weight-gradient GEMMs (main stream only)
    int64_t o_lsws = 0, lsws_floats = 0;  // S | T scratch of the z-free LayerScale gradient
    bool det = false;                     // created in deterministic mode (lnx_set_deterministic): scratch and kernel choice fit its fixed-order routes
    int64_t o_detws = 0, detws_floats = 0;  // ... the partial sums of the depthwise weight gradient / the LayerScale gradient (launch stream, one at a time)
    int64_t o_gcos /* freqs-gradient partials of lnx_attn_bwd */, o_delta, o_dt1, o_tail[6], o_mtmp[4], o_dlT;
    // fp8 plans, forward scratch: MXFP8 copy (+ block scales) of the LayerNorm output feeding qkv / fc1, and of the MLP hidden
    // feeding fc2 (two buffers: fc1 reads the first while its epilogue writes the second)
    int64_t o_a8 = 0, o_a8s = 0, o_h8 = 0, o_h8s = 0;
    const float* last_drop = nullptr;
    const unsigned char* last_mask = nullptr;
    std::vector<unsigned char> mask_host;
    const float* last_meta = nullptr;
    // recompute plans: index of the block whose activations currently sit in each stage's shared buffer set
    int resident[4] = {-1, -1, -1, -1};
    // training-time dropout of the RoPE blocks (lnx_plan_set_dropout): caller-owned keep masks, 1 / (1 - drop_rate)
    const unsigned char* dmask = nullptr;
    float inv_keep = 1.0f;
    int64_t dmask_bytes = 0;
    const unsigned char* amask = nullptr;  // attention-probability dropout (lnx_plan_set_attn_dropout)
    float a_inv_keep = 1.0f;
    int64_t amask_bytes = 0;
    // side stream for the tiny M = batch metadata-head chains: they are independent of the image path
    // until token assembly, so they run concurrently with the conv stages (forward) / the downsample
    // backward (backward) instead of serialising ~100 small launches on the main stream
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_meta = nullptr, ev_bfork[2] = {nullptr, nullptr}, ev_bjoin[2] = {nullptr, nullptr};
    // Weight-gradient stream (round 4; LNX_WGRAD_STREAM=0 / lnx_plan_set_wgrad_stream(p, 0): everything on the launch stream): the
    // RoPE blocks' four weight-gradient products + their batched reduce, and the fused ConvNeXt blocks' two + the LayerScale step, run on a
    // stream of their own beside the data-gradient chain / the depthwise backward.  Each product forks behind the kernel that wrote its dY
    // and is joined before that buffer's next writer; every block ends with a join, so a segment's gradients are complete when it returns.
    // The kernels do not share CUs (one workgroup per CU by LDS) -- what overlaps is one kernel's ramp and tail with the other's body.
    hipStream_t wgs = nullptr;
    bool wgs_on = true;
    bool meta_forked[2] = {false, false};  // backward: stage s's metadata heads were forked off the launch stream and not joined yet
    int meta_mode = 1;       // which stream the metadata heads run on: 0 launch stream, 1 their own side stream, 2 the weight-gradient stream (lnx_plan_set_meta_stream)
    bool meta_chain = true;  // metadata heads as one launch per direction (metahead.hip); LNX_META_CHAIN=0: the round-1 chain of GEMM / LayerNorm launches (A/B)
    bool chain_ok[2] = {false, false};  // ... per RoPE stage: the one-launch chain carries widths up to 1024 (lnx_meta_heads_supported)
    bool dy8_ready = false;  // backward, fp8 plans: o_a8 / o_a8s hold the MXFP8 copy of the dY in sC (written by the LayerNorm backward that wrote sC)
    hipEvent_t ev_wf[4] = {nullptr, nullptr, nullptr, nullptr}, ev_wj[4] = {nullptr, nullptr, nullptr, nullptr};
    // optional per-kernel-class timing with HIP events (bench.py's live roofline measurement)
    bool profile = false;
    bool profile_spans = false;  // block-level spans only (classes 8 / 9: whole RoPE / ConvNeXt blocks), no per-launch events
    struct Span { hipEvent_t e0, e1; int cls; double work, bytes; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;

    template <typename U> U* at(int64_t off) const { return reinterpret_cast<U*>(ws + off); }
    const float* drop_ptr(int call) const {
        if (last_drop == nullptr || call < 0 || !mask_host[call]) return nullptr;
        return last_drop + (int64_t)call * c.batch;
    }
    // DropPath compaction: the lists lnx_plan_forward built for the RoPE blocks' drop calls of this forward, n_drop regions of
    // LNX_DROP_LIST_INTS(batch) ints; valid until the next forward (the backward and a recompute plan's re-forward read them).  A device
    // allocation of the plan's own (a few KiB, made by the first forward that compacts, freed by lnx_plan_destroy): the caller's
    // workspace keeps its size.
    int* droplists = nullptr;
    bool compact_now = false;
    bool compact_conv_now = false;  // ... and the conv blocks' calls are among them (LNX_DROP_COMPACT_CONV)
    // CLS-only last block: the last forward ran the last stage-4 block's proj / norm2 / MLP on the B CLS rows only (norm_2 reads
    // nothing else of the stage output); the backward and a recompute plan's re-forward follow that forward's choice
    bool last_cls_now = false;
    // Metadata variants: the last lnx_plan_forward of this inference plan completed and nothing has touched what it left in front
    // of the token boundary (the stage-3 patch and CLS rows in o_tok[0], the operand arena, the cos / sin tables): lnx_plan_forward_tail may
    // re-run the token stages with other metadata.  Cleared on entry to lnx_plan_forward, by lnx_plan_bind and by any failed call.
    bool trunk_valid = false;
    bool last_cls(int s, int i) const { return last_cls_now && s == 1 && i + 1 == (int)rope[1].size(); }
    const int* drop_list(int call) const {
        if (!compact_now || droplists == nullptr || drop_ptr(call) == nullptr) return nullptr;
        return droplists + (int64_t)call * LNX_DROP_LIST_INTS(c.batch);
    }
};

// A/B switch of the DropPath compaction, process-wide: -1 = LNX_DROP_COMPACT (on unless set to 0), else what lnx_set_drop_compact said
static std::atomic<int> g_drop_compact{-1};
static std::atomic<long long> g_compact_branches{0};
extern "C" int lnx_set_drop_compact(int on) {
    const int was = g_drop_compact.exchange(on < 0 ? -1 : (on ? 1 : 0));
    return was;
}
extern "C" int64_t lnx_drop_compact_branches(void) { return (int64_t)g_compact_branches.load(std::memory_order_relaxed); }
static std::atomic<long long> g_compact_conv_blocks{0};
extern "C" int64_t lnx_drop_compact_conv_blocks(void) { return (int64_t)g_compact_conv_blocks.load(std::memory_order_relaxed); }
// A/B switch of the CLS-only last RoPE block, process-wide: -1 = LNX_LAST_CLS (on unless set to 0), else what lnx_set_last_cls said
static std::atomic<int> g_last_cls{-1};
static std::atomic<long long> g_last_cls_blocks{0};
extern "C" int lnx_set_last_cls(int on) { return g_last_cls.exchange(on < 0 ? -1 : (on ? 1 : 0)); }
extern "C" int64_t lnx_last_cls_blocks(void) { return (int64_t)g_last_cls_blocks.load(std::memory_order_relaxed); }

namespace {

bool env_set(const char* name) { return getenv(name) != nullptr; }
bool env_off(const char* name) {  // the A/B switches that default to on: set and equal to 0
    const char* e = getenv(name);
    return e != nullptr && atoi(e) == 0;
}

OpW make_w(lnx_plan* p, int param, int N, int K, bool want_t, int mode = LNX_PREP_CAST, int P = 0, bool f32 = false) {
    OpW w;
    w.param = param;
    w.N = N;
    w.K = K;
    w.f32 = f32 || p->esz == 4;
    const int epv = w.f32 ? 4 : 8;
    w.ld = (int)align_up(K, epv);
    if (K < 16) w.ld = 16;  // tiny-K first meta Linear: pad to one 16-element chunk row
    w.ld_t = want_t ? (int)align_up(N, epv) : 0;
    w.mode = mode;
    w.P = P;
    return w;
}

// The parameters, once: inventory in the reference's state_dict order (mFormerV1.py:145-343; checked against the reference by
// tests/golden/gen/make_golden.py through oracle.param_shapes), the handle of each in the plan, its operand-arena entry if it is a
// GEMM weight, and the backward segment that finishes its gradient: 0 tail + stage 4 + downsample 3, 1 stage 3 + downsample 2,
// 2 ConvNeXt stage 2 + downsample 1, 3 ConvNeXt stage 1 + stem.
void build_params(lnx_plan* p) {
    const lnx_mformer_cfg& c = p->c;
    const int* D = c.dims;
    const int B = c.batch;
    char b[128];
    auto add = [&](const std::string& name, int64_t numel, int seg) {
        p->names.push_back(name);
        p->numel.push_back(numel);
        p->seg.push_back((signed char)seg);
        return (int)p->names.size() - 1;
    };
    p->cls[0] = add("cls_token_1", D[2], 1);
    p->cls[1] = add("cls_token_2", D[3], 0);
    p->stem_w = make_w(p, add("stem.0.weight", (int64_t)D[0] * c.in_chans * 16, 3), D[0], c.in_chans * 16, false);
    p->stem_w.ld = 64;
    p->stem_b = add("stem.0.bias", D[0], 3);
    p->stem_lnw = add("stem.1.weight", D[0], 3);
    p->stem_lnb = add("stem.1.bias", D[0], 3);
    for (int i = 0; i < 3; ++i) {
        snprintf(b, sizeof b, "downsample_layers.%d.", i);
        const std::string pre(b);
        Down& k = p->down[i];
        const int seg = 2 - i;
        k.lnw = add(pre + "norm.weight", D[i], seg);
        k.lnb = add(pre + "norm.bias", D[i], seg);
        k.w = make_w(p, add(pre + "conv.weight", (int64_t)D[i + 1] * D[i] * 4, seg), D[i + 1], 4 * D[i], true, LNX_PREP_CONV_PERM, 4);
        k.cb = add(pre + "conv.bias", D[i + 1], seg);
    }
    int call = 0;  // DropPath calls in forward order: the conv blocks, then per RoPE block the attention branch and the MLP branch
    for (int s = 0; s < 2; ++s) {
        p->conv[s].resize(c.conv_depths[s]);
        for (int i = 0; i < c.conv_depths[s]; ++i) {
            snprintf(b, sizeof b, "stages.%d.%d.", s, i);
            const std::string pre(b);
            ConvBlk& k = p->conv[s][i];
            const int C = D[s], seg = 3 - s;
            k.gamma = add(pre + "gamma", C, seg);
            k.dww = add(pre + "dwconv.weight", (int64_t)C * 49, seg);
            k.dwb = add(pre + "dwconv.bias", C, seg);
            k.lnw = add(pre + "norm.weight", C, seg);
            k.lnb = add(pre + "norm.bias", C, seg);
            k.w1 = make_w(p, add(pre + "pwconv1.weight", (int64_t)4 * C * C, seg), 4 * C, C, true);
            k.b1 = add(pre + "pwconv1.bias", 4 * C, seg);
            k.w2 = make_w(p, add(pre + "pwconv2.weight", (int64_t)4 * C * C, seg), C, 4 * C, true);
            k.b2 = add(pre + "pwconv2.bias", C, seg);
            p->drop_conv[s].push_back(call++);
        }
    }
    for (int s = 0; s < 2; ++s) {
        p->rope[s].resize(c.rope_depths[s]);
        for (int i = 0; i < c.rope_depths[s]; ++i) {
            snprintf(b, sizeof b, "stages.%d.%d.", s + 2, i);
            const std::string pre(b);
            RopeBlk& k = p->rope[s][i];
            const int C = D[2 + s], hid = c.mlp_hidden[s], seg = 1 - s;
            k.n1w = add(pre + "norm1.weight", C, seg);
            k.n1b = add(pre + "norm1.bias", C, seg);
            k.n2w = add(pre + "norm2.weight", C, seg);
            k.n2b = add(pre + "norm2.bias", C, seg);
            k.freqs = add(pre + "attn.freqs", C, seg);  // [2, heads, head_dim / 2]: 2 * heads * head_dim / 2 = C
            k.qkv = make_w(p, add(pre + "attn.qkv.weight", (int64_t)3 * C * C, seg), 3 * C, C, true);
            k.qkvb = add(pre + "attn.qkv.bias", 3 * C, seg);
            k.proj = make_w(p, add(pre + "attn.proj.weight", (int64_t)C * C, seg), C, C, true);
            k.projb = add(pre + "attn.proj.bias", C, seg);
            k.fc1 = make_w(p, add(pre + "mlp.fc1.weight", (int64_t)hid * C, seg), hid, C, true);
            k.fc1b = add(pre + "mlp.fc1.bias", hid, seg);
            k.fc2 = make_w(p, add(pre + "mlp.fc2.weight", (int64_t)C * hid, seg), C, hid, true);
            k.fc2b = add(pre + "mlp.fc2.bias", C, seg);
            p->drop_attn[s].push_back(call++);
            p->drop_mlp[s].push_back(call++);
        }
    }
    p->n_drop = call;
    for (int s = 0; s < 2; ++s) {
        snprintf(b, sizeof b, "norm_%d.", s + 1);
        p->norm_w[s] = add(std::string(b) + "weight", D[2 + s], 0);
        p->norm_b[s] = add(std::string(b) + "bias", D[2 + s], 0);
        p->meta[s].resize(c.n_meta);
    }
    int off = 0;  // a component's columns in the metadata row: the prefix sum of meta_dims
    for (int m = 0; m < c.n_meta; ++m) {
        for (int s = 0; s < 2; ++s) {
            snprintf(b, sizeof b, "meta.%d.head_%d.", m, s + 1);
            const std::string pre(b);
            MetaHead& k = p->meta[s][m];
            // metadata heads run beside the launch stream and are joined one segment after the one that forks them
            const int C = D[2 + s], seg = 2 - s;
            k.dim = c.meta_dims[m];
            k.off = off;
            k.w0 = make_w(p, add(pre + "0.weight", (int64_t)C * k.dim, seg), C, k.dim, false, LNX_PREP_CAST, 0, true);
            k.b0 = add(pre + "0.bias", C, seg);
            k.lnw0 = add(pre + "2.weight", C, seg);
            k.lnb0 = add(pre + "2.bias", C, seg);
            k.nf1w = add(pre + "3.norm_fn1.weight", C, seg);
            k.nf1b = add(pre + "3.norm_fn1.bias", C, seg);
            k.nf2w = add(pre + "3.norm_fn2.weight", C, seg);
            k.nf2b = add(pre + "3.norm_fn2.bias", C, seg);
            k.w1 = make_w(p, add(pre + "3.w1.weight", (int64_t)C * C, seg), C, C, true, LNX_PREP_CAST, 0, true);
            k.b1 = add(pre + "3.w1.bias", C, seg);
            k.w2 = make_w(p, add(pre + "3.w2.weight", (int64_t)C * C, seg), C, C, true, LNX_PREP_CAST, 0, true);
            k.b2 = add(pre + "3.w2.bias", C, seg);
        }
        off += c.meta_dims[m];
    }
    if (!c.only_last_cls) {
        p->cl_w1 = make_w(p, add("cl_1_fc.0.fc1.weight", (int64_t)D[2] * D[2], 0), D[2], D[2], true);
        p->cl_b1 = add("cl_1_fc.0.fc1.bias", D[2], 0);
        p->cl_w2 = make_w(p, add("cl_1_fc.0.fc2.weight", (int64_t)D[3] * D[2], 0), D[3], D[2], true);
        p->cl_b2 = add("cl_1_fc.0.fc2.bias", D[3], 0);
        p->cl_lnw = add("cl_1_fc.1.weight", D[3], 0);
        p->cl_lnb = add("cl_1_fc.1.bias", D[3], 0);
        p->agg_w = add("aggregate.weight", 2, 0);
        p->agg_b = add("aggregate.bias", 1, 0);
    }
    p->fin_w = add("final_norm.weight", D[3], 0);
    p->fin_b = add("final_norm.bias", D[3], 0);
    p->head_w.resize(c.n_tasks);
    p->head_b.resize(c.n_tasks);
    p->logit_ld.resize(c.n_tasks);
    p->logit_off.resize(c.n_tasks);
    for (int t = 0; t < c.n_tasks; ++t) {
        snprintf(b, sizeof b, "head.%d.", t);
        p->head_w[t] = make_w(p, add(std::string(b) + "weight", (int64_t)c.task_classes[t] * D[3], 0), c.task_classes[t], D[3], true);
        p->head_b[t] = add(std::string(b) + "bias", c.task_classes[t], 0);
        p->logit_ld[t] = (int)align_up(c.task_classes[t], 8);
        p->head_w[t].ld_t = p->logit_ld[t];  // the data-gradient GEMM contracts over the padded logits row
        p->logit_off[t] = p->logits_numel;
        p->logits_numel += (int64_t)B * p->logit_ld[t];
    }
}

// The unit list in forward order and the unit of every parameter, by name: "stem", "stages.<s>.<i>", "downsample_layers.0|1", "tokens_1|2"
// (cls_token_k and every metadata head of stage k), "mid" (norm_1, cl_1_fc, downsample_layers.2), "tail" (norm_2, aggregate, final_norm),
// "heads".  Returns false on a parameter name it cannot place (a parameter added to build_params without a unit).
bool build_units(lnx_plan* p) {
    const lnx_mformer_cfg& c = p->c;
    char b[64];
    auto unit = [&](const std::string& name) {
        p->unit_names.push_back(name);
        return (int)p->unit_names.size() - 1;
    };
    auto blocks = [&](int stage, int depth) {
        const int first = (int)p->unit_names.size();
        for (int i = 0; i < depth; ++i) {
            snprintf(b, sizeof b, "stages.%d.%d", stage, i);
            unit(b);
        }
        return first;
    };
    unit("stem");
    for (int s = 0; s < 2; ++s) {
        p->u_conv[s] = blocks(s, c.conv_depths[s]);
        snprintf(b, sizeof b, "downsample_layers.%d", s);
        p->u_down[s] = unit(b);
    }
    p->u_tok[0] = unit("tokens_1");
    p->u_rope[0] = blocks(2, c.rope_depths[0]);
    p->u_mid = unit("mid");
    p->u_tok[1] = unit("tokens_2");
    p->u_rope[1] = blocks(3, c.rope_depths[1]);
    p->u_tail = unit("tail");
    p->u_heads = unit("heads");
    auto starts = [](const std::string& s, const char* pre) { return s.compare(0, strlen(pre), pre) == 0; };
    p->unit_of.assign(p->names.size(), -1);
    for (size_t i = 0; i < p->names.size(); ++i) {
        const std::string& n = p->names[i];
        int u = -1, s = 0, k = 0, m = 0;
        if (starts(n, "stem.")) u = 0;
        else if (sscanf(n.c_str(), "stages.%d.%d.", &s, &k) == 2 && s >= 0 && s < 4) u = (s < 2 ? p->u_conv[s] : p->u_rope[s - 2]) + k;
        else if (sscanf(n.c_str(), "downsample_layers.%d.", &s) == 1) u = s < 2 ? p->u_down[s] : p->u_mid;
        else if (sscanf(n.c_str(), "cls_token_%d", &s) == 1 && (s == 1 || s == 2)) u = p->u_tok[s - 1];
        else if (sscanf(n.c_str(), "meta.%d.head_%d.", &m, &s) == 2 && (s == 1 || s == 2)) u = p->u_tok[s - 1];
        else if (starts(n, "norm_1.") || starts(n, "cl_1_fc.")) u = p->u_mid;
        else if (starts(n, "norm_2.") || starts(n, "aggregate.") || starts(n, "final_norm.")) u = p->u_tail;
        else if (starts(n, "head.")) u = p->u_heads;
        if (u < 0 || u >= (int)p->unit_names.size()) return false;
        p->unit_of[i] = u;
    }
    return true;
}

struct Carver {
    int64_t cur = 0;
    int64_t take(int64_t bytes) {
        const int64_t o = cur;
        cur += align_up(bytes > 0 ? bytes : 16, 256);
        return o;
    }
};

}  // namespace

static void layout_workspace(lnx_plan* p);
static void apply_cut(lnx_plan* p);

extern "C" int lnx_plan_create(const lnx_mformer_cfg* cfg, lnx_plan** out) {
    if (!cfg || !out) FAIL("lnx_plan_create: null argument");
    const lnx_mformer_cfg& c = *cfg;
    if (c.dtype != LNX_F32 && c.dtype != LNX_BF16) FAIL("lnx_plan_create: bad dtype %d", c.dtype);
    if (c.batch <= 0 || c.img_h <= 0 || c.img_w <= 0 || c.in_chans <= 0 || c.in_chans > 4) FAIL("lnx_plan_create: bad input geometry");
    if (c.img_h % 32 != 0 || c.img_w % 32 != 0) FAIL("lnx_plan_create: image size %dx%d must be divisible by 32 (4*2*2*2 patchify)", c.img_h, c.img_w);
    for (int i = 0; i < 4; ++i)
        if (c.dims[i] <= 0 || c.dims[i] % 32 != 0 || c.dims[i] > 2048) FAIL("lnx_plan_create: dims[%d]=%d must be a multiple of 32 in (0, 2048]", i, c.dims[i]);
    for (int s = 0; s < 2; ++s) {
        if (c.conv_depths[s] < 0 || c.rope_depths[s] <= 0) FAIL("lnx_plan_create: bad depths");
        const int hd = c.rope_heads[s] > 0 && c.dims[2 + s] % c.rope_heads[s] == 0 ? c.dims[2 + s] / c.rope_heads[s] : 0;
        if (hd != 32 && hd != 64 && hd != 128)
            FAIL("lnx_plan_create: head_dim = dim / heads must be 32, 64 or 128 (dim %d, heads %d)", c.dims[2 + s], c.rope_heads[s]);
        if (c.mlp_hidden[s] <= 0 || c.mlp_hidden[s] % 16 != 0) FAIL("lnx_plan_create: mlp_hidden must be a multiple of 16");
    }
    if (c.n_meta < 0 || c.n_meta > LNX_MAX_META || c.n_tasks < 0 || c.n_tasks > LNX_MAX_TASKS) FAIL("lnx_plan_create: too many meta components / tasks");
    for (int m = 0; m < c.n_meta; ++m)
        if (c.meta_dims[m] <= 0 || c.meta_dims[m] > 16) FAIL("lnx_plan_create: meta dim %d must be in 1..16", c.meta_dims[m]);
    if (c.rope_mode != LNX_ROPE_COS && c.rope_mode != LNX_ROPE_ROTATE) FAIL("lnx_plan_create: rope_mode %d (LNX_ROPE_COS or LNX_ROPE_ROTATE)", c.rope_mode);

    if (c.fp8) {
        if (c.dtype != LNX_BF16) FAIL("lnx_plan_create: fp8 = 1 needs dtype = LNX_BF16 (fp8 operands, bf16 storage)");
        for (int s = 0; s < 2; ++s)
            if (c.dims[2 + s] % 128 != 0 || c.mlp_hidden[s] % 128 != 0)
                FAIL("lnx_plan_create: fp8 = 1 needs RoPE dims and MLP widths that are multiples of 128 (stage %d: %d / %d)", s + 2, c.dims[2 + s], c.mlp_hidden[s]);
    }
    lnx_plan* p = new lnx_plan();
    p->c = c;
    p->esz = c.dtype == LNX_BF16 ? 2 : 4;
    p->meta_chain = !env_off("LNX_META_CHAIN");
    p->ln_defer = !env_off("LNX_LN_DEFER");
    p->det = lnx_get_deterministic() != 0;
    p->freq_defer = !env_off("LNX_FREQ_DEFER");
    for (int s = 0; s < 2; ++s) p->chain_ok[s] = p->meta_chain && lnx_meta_heads_supported(c.dims[2 + s]) != 0;
    p->E = 1 + c.n_meta;
    p->H[0] = c.img_h / 4;
    p->W[0] = c.img_w / 4;
    for (int i = 1; i < 4; ++i) {
        p->H[i] = p->H[i - 1] / 2;
        p->W[i] = p->W[i - 1] / 2;
    }
    for (int i = 0; i < 4; ++i) p->HW[i] = p->H[i] * p->W[i];
    for (int s = 0; s < 2; ++s) p->Ntok[s] = p->HW[2 + s] + p->E;
    build_params(p);
    p->frozen_prefix = !env_off("LNX_FROZEN_PREFIX");
    if (!build_units(p)) {
        delete p;
        FAIL("lnx_plan_create: a parameter without a unit (build_units does not know its name)");
    }

    // collect every arena weight
    auto reg = [&](OpW& w) { p->all_w.push_back(&w); };
    reg(p->stem_w);
    for (int i = 0; i < 3; ++i) reg(p->down[i].w);
    for (int s = 0; s < 2; ++s)
        for (auto& k : p->conv[s]) {
            reg(k.w1);
            reg(k.w2);
        }
    for (int s = 0; s < 2; ++s)
        for (auto& k : p->rope[s]) {
            reg(k.qkv);
            reg(k.proj);
            reg(k.fc1);
            reg(k.fc2);
        }
    for (int s = 0; s < 2; ++s)
        for (auto& k : p->meta[s]) {
            reg(k.w0);
            reg(k.w1);
            reg(k.w2);
        }
    if (!c.only_last_cls) {
        reg(p->cl_w1);
        reg(p->cl_w2);
    }
    for (auto& w : p->head_w) reg(w);
    layout_workspace(p);
    *out = p;
    return 0;
}

// The workspace layout for the plan's cut (lnx_plan::cut; 0 = every unit trains: the layout of a plan without frozen units).  Run by
// lnx_plan_create and again by lnx_plan_set_trainable: every offset and size is assigned here, nothing accumulates across runs.
static void layout_workspace(lnx_plan* p) {
    const lnx_mformer_cfg& c = p->c;
    const int* D = c.dims;
    const int B = c.batch;
    const int esz = p->esz;
    const int cut = p->cut;
    p->dmask_bytes = p->amask_bytes = 0;
    p->detws_floats = 0;
    Carver cv;
    int ndw = 0;
    for (int s = 0; s < 2; ++s) ndw += c.conv_depths[s];
    p->n_descs = (int64_t)p->all_w.size() + ndw;
    p->o_descs = cv.take(p->n_descs * sizeof(lnx_prep_desc));
    for (OpW* w : p->all_w) {
        const int wes = w->f32 ? 4 : 2;
        w->off = cv.take((int64_t)w->N * w->ld * wes);
        if (w->ld_t) w->off_t = cv.take((int64_t)w->K * w->ld_t * wes);
    }
    p->arena_end = cv.cur;
    for (int s = 0; s < 2; ++s)
        for (auto& k : p->conv[s]) k.w49 = cv.take((int64_t)49 * D[s] * 4);
    if (c.fp8) {
        const bool fp8_dgrad = !c.inference && !env_off("LNX_FP8_DGRAD");
        for (int s = 0; s < 2; ++s)
            for (auto& k : p->rope[s]) {
                for (OpW* w : {&k.qkv, &k.fc1, &k.fc2}) {
                    w->off8 = cv.take((int64_t)w->N * w->K);
                    w->off8s = cv.take((int64_t)(w->K / 128) * w->N * 4);
                }
                // The proj / fc2 / fc1 data-gradient products in MXFP8 too (round 5: on by default, LNX_FP8_DGRAD=0 keeps them bf16).  Global
                // gradient error against the fp32 oracle 8.7 % instead of 6.9 % (sm, B = 24) -- inside the mode's stated 12-13 % -- for
                // 84.6 instead of 85.7 ms per xl step (round 4); dY arrives as the MXFP8 copy the LayerNorm backward writes beside its bf16 output.
                if (fp8_dgrad)
                    for (OpW* w : {&k.proj, &k.fc1, &k.fc2}) {
                        w->off8t = cv.take((int64_t)w->K * w->N);
                        w->off8ts = cv.take((int64_t)(w->N / 128) * w->K * 4);
                    }
            }
    }

    const int64_t M0 = (int64_t)B * p->HW[0];
    p->o_patches = cv.take(M0 * 64 * esz);
    p->o_stem_pre = cv.take(M0 * D[0] * esz);
    p->o_stem_mean = cv.take(M0 * 4);
    p->o_stem_rstd = cv.take(M0 * 4);
    int64_t maxMC = 0, maxM4C = 0;
    int64_t fwdMC = 0;  // what the FORWARD writes into sD: with dropout masks bound, the proj / fc2 product of every RoPE block, frozen or not
    bool any_fused = false;
    // Inference plans: nothing is saved for a backward, so the blocks of a stage share one set of activation buffers
    // and the residual stream ping-pongs between two (the workspace no longer grows with the depth).
    // Recompute plans (cfg.recompute, training): the same sharing, but every block keeps its own INPUT; the backward
    // re-runs a block's forward into the shared set before differentiating it.
    const bool inf = c.inference != 0;
    const bool ck = !inf && c.recompute != 0;
    // LNX_NO_FUSED_MLP: every conv block on two GEMMs; LNX_FUSED_MLP_MAXC=n: only blocks with C <= n fused; LNX_NO_FUSED_LN: the block
    // LayerNorm as its own passes again (A/B switches)
    const bool fuse_mlp = !env_set("LNX_NO_FUSED_MLP"), fuse_ln = !env_set("LNX_NO_FUSED_LN");
    int fuse_maxc = 2048;  // (no dims[] is larger)
    if (const char* e = getenv("LNX_FUSED_MLP_MAXC")) fuse_maxc = atoi(e);
    p->lnws_floats = (int64_t)2048 * 2 * (D[3] > D[0] ? D[3] : D[0]);
    p->lnws_side_floats = (int64_t)256 * 2 * D[3];
    if (p->det)  // the fused conv-MLP backward then leaves a row per WAVE: room for the largest conv stage, so it keeps the LayerNorm inside
        for (int s = 0; s < 2; ++s) {
            const int64_t need = lnx_convmlp_bwd_ws_floats((int)D[s], (int)((int64_t)B * p->HW[s]));
            if (need > p->lnws_floats) p->lnws_floats = need;
        }
    // Frozen prefix (cut > 0, training plans): the nf blocks of a stage that lie before the cut run forward-only.  They share one set of
    // activation buffers (block 0's), and the fp32 stream through them ping-pongs between two buffers; the input of the first trained
    // block is the last buffer they wrote and stays valid (every later block writes a buffer of its own).  The backward scratch is sized
    // by the stages whose units still run a backward.  With cut == 0 nothing below differs from the plan without frozen units.
    auto frozen_blocks = [&](int first_unit, size_t nb) {  // blocks of a stage before the cut: cut - first_unit, clamped to [0, nb]
        if (inf || cut <= first_unit) return 0;
        return cut - first_unit < (int)nb ? cut - first_unit : (int)nb;
    };
    for (int s = 0; s < 2; ++s) {
        const int64_t M = (int64_t)B * p->HW[s], C = D[s];
        const bool active = cut <= p->u_down[s];  // a unit of this stage's row count (s == 0: the stem too) runs a backward
        if (active && M * C > maxMC) maxMC = M * C;
        if (active && M * 4 * C > maxM4C) maxM4C = M * 4 * C;
        int64_t pp[2] = {0, 0};
        if (inf) {
            pp[0] = cv.take(M * C * 4);
            pp[1] = cv.take(M * C * 4);
        }
        const size_t nb = p->conv[s].size();
        const int nf = frozen_blocks(p->u_conv[s], nb);
        // fp32 stream buffer k of the stage (k < nb: input of block k; k == nb: the stage output)
        auto stream_buf = [&](size_t k) {
            if (inf) return pp[k & 1];
            if ((int)k > nf) return cv.take(M * C * 4);
            if (pp[k & 1] == 0) pp[k & 1] = cv.take(M * C * 4);
            return pp[k & 1];
        };
        for (size_t i = 0; i < nb; ++i) {
            ConvBlk& k = p->conv[s][i];
            const bool share = i > 0 && (inf || ck || (int)i < nf);
            const ConvBlk& f = p->conv[s][0];
            k.xin = stream_buf(i);
            k.y = share ? f.y : cv.take(M * C * esz);
            k.ln = share ? f.ln : cv.take(M * C * esz);
            k.mean = share ? f.mean : cv.take(M * 4);
            k.rstd = share ? f.rstd : cv.take(M * 4);
            k.fused = lnx_convmlp_supported(c.dtype, (int)C) != 0 && fuse_mlp && C <= fuse_maxc;
            any_fused = any_fused || k.fused;
            // The backward kernel leaves 2C floats of column sums per workgroup in the LayerNorm scratch; how many workgroups is the
            // launcher's business (lnx_convmlp_bwd_ws_floats), a batch whose sums do not fit keeps the separate LayerNorm passes.
            k.fused_ln = k.fused && fuse_ln && lnx_convmlp_bwd_ws_floats((int)C, (int)M) <= p->lnws_floats;
            if (!k.fused) {
                k.hpre = share ? f.hpre : cv.take(M * 4 * C * esz);
                k.act = share ? f.act : cv.take(M * 4 * C * esz);
                k.z = share ? f.z : cv.take(M * C * esz);
            }
        }
        p->o_stage_out[s] = stream_buf(nb);
        p->down[s].ln = cv.take(M * C * esz);
        p->down[s].mean = cv.take(M * 4);
        p->down[s].rstd = cv.take(M * 4);
        p->o_g[s] = inf || !active ? 0 : cv.take(M * C * 4);
    }
    for (int s = 0; s < 2; ++s) {
        const int N = p->Ntok[s];
        const int64_t M = (int64_t)B * N, C = D[2 + s], hid = c.mlp_hidden[s];
        const int heads = c.rope_heads[s];
        // a unit of this stage's row count runs a backward: its blocks, and for stage 3 `mid` behind it (norm_1, downsample 3)
        const bool active = s == 0 ? cut <= p->u_mid : cut < p->u_tail;
        if (active && M * C > maxMC) maxMC = M * C;
        if (M * C > fwdMC) fwdMC = M * C;
        const int64_t wide = hid > 3 * C ? hid : 3 * C;
        if (active && M * wide > maxM4C) maxM4C = M * wide;
        p->o_tok[s] = cv.take(M * C * 4);
        int64_t pp[2] = {0, 0};
        if (inf) {
            pp[0] = cv.take(M * C * 4);
            pp[1] = cv.take(M * C * 4);
        }
        const int nf = frozen_blocks(p->u_rope[s], p->rope[s].size());
        for (size_t i = 0; i < p->rope[s].size(); ++i) {
            RopeBlk& k = p->rope[s][i];
            const bool share = i > 0 && (inf || ck || (int)i < nf);
            const RopeBlk& f = p->rope[s][0];
            if (i == 0) k.xin = p->o_tok[s];  // later blocks: output buffer of the previous block (set below)
            k.n1 = share ? f.n1 : cv.take(M * C * esz);
            k.mean1 = share ? f.mean1 : cv.take(M * 4);
            k.rstd1 = share ? f.rstd1 : cv.take(M * 4);
            k.qkvbuf = share ? f.qkvbuf : cv.take(M * 3 * C * esz);
            k.cos = cv.take((int64_t)p->HW[2 + s] * C / 2 * 4);  // [HW, heads, head_dim / 2]
            // d cos / d freqs, for the attention backward; rotate plans (forward and backward) keep sin(theta), one table, in its place
            if (c.rope_mode == LNX_ROPE_ROTATE) k.dsin = cv.take((int64_t)p->HW[2 + s] * C / 2 * 4);
            else k.dsin = inf ? 0 : cv.take((int64_t)2 * p->HW[2 + s] * C / 2 * 4);
            k.o = share ? f.o : cv.take(M * C * esz);
            k.lse = share ? f.lse : cv.take((int64_t)B * heads * N * 4);
            k.xmid = share ? f.xmid : cv.take(M * C * 4);
            k.n2 = share ? f.n2 : cv.take(M * C * esz);
            k.mean2 = share ? f.mean2 : cv.take(M * 4);
            k.rstd2 = share ? f.rstd2 : cv.take(M * 4);
            k.hpre = share ? f.hpre : cv.take(M * hid * esz);
            k.act = share ? f.act : cv.take(M * hid * esz);
            int64_t outb = 0;
            if (inf) outb = pp[i & 1];
            else if ((int)i < nf) outb = pp[i & 1] ? pp[i & 1] : (pp[i & 1] = cv.take(M * C * 4));  // a frozen block's output: ping-pong
            else outb = cv.take(M * C * 4);
            if (i + 1 < p->rope[s].size()) p->rope[s][i + 1].xin = outb;
            else p->o_stage_out[2 + s] = outb;
        }
        // the gradient stream of the stage: written from norm_1's (s == 0) / norm_2's (s == 1) backward on
        p->o_g[2 + s] = inf || cut > (s == 0 ? p->u_mid : p->u_tail) ? 0 : cv.take(M * C * 4);
        for (auto& k : p->meta[s]) {
            // meta heads run in fp32 storage in both modes (M = batch rows: negligible cost)
            k.t0 = cv.take((int64_t)B * 16 * 4);
            k.h0 = cv.take((int64_t)B * C * 4);
            k.x = cv.take((int64_t)B * C * 4);
            k.m0 = cv.take(B * 4);
            k.r0 = cv.take(B * 4);
            k.h1 = cv.take((int64_t)B * C * 4);
            k.n1 = cv.take((int64_t)B * C * 4);
            k.m1 = cv.take(B * 4);
            k.r1 = cv.take(B * 4);
            k.h2 = cv.take((int64_t)B * C * 4);
            k.m2 = cv.take(B * 4);
            k.r2 = cv.take(B * 4);
            if (!inf && p->chain_ok[s] && cut <= p->u_tok[s]) {  // the heads of a stage run side by side in one launch: backward scratch per head
                k.dp2 = cv.take((int64_t)B * C * 4);
                k.dp1 = cv.take((int64_t)B * C * 4);
                k.dp0 = cv.take((int64_t)B * C * 4);
                k.part = cv.take(lnx_meta_heads_bwd_part_floats(B, (int)C) * 4);
            }
        }
    }
    {
        const int64_t M2 = (int64_t)B * p->Ntok[0];
        p->o_t1 = cv.take(M2 * D[2] * esz);
        p->o_t1_mean = cv.take(M2 * 4);
        p->o_t1_rstd = cv.take(M2 * 4);
        p->o_dt1 = inf || cut > p->u_mid ? 0 : cv.take(M2 * D[2] * esz);
        p->down[2].ln = cv.take((int64_t)B * p->HW[2] * D[2] * esz);
        p->down[2].mean = cv.take((int64_t)B * p->HW[2] * 4);
        p->down[2].rstd = cv.take((int64_t)B * p->HW[2] * 4);
        p->o_cl_hpre = cv.take((int64_t)B * D[2] * esz);
        p->o_cl_act = cv.take((int64_t)B * D[2] * esz);
        p->o_cl_u = cv.take((int64_t)B * D[3] * 4);
        p->o_cl_mean = cv.take(B * 4);
        p->o_cl_rstd = cv.take(B * 4);
        p->o_c1n = cv.take((int64_t)B * D[3] * 4);
        p->o_c2n = cv.take((int64_t)B * D[3] * 4);
        p->o_n2_mean = cv.take(B * 4);
        p->o_n2_rstd = cv.take(B * 4);
        p->o_agg = cv.take((int64_t)B * D[3] * 4);
        p->o_fin_mean = cv.take(B * 4);
        p->o_fin_rstd = cv.take(B * 4);
        p->o_feats = cv.take((int64_t)B * D[3] * 4);
        p->o_featsT = cv.take((int64_t)B * D[3] * esz);
        for (int i = 0; i < 6; ++i) p->o_tail[i] = cv.take((int64_t)B * D[3] * 4);
        for (int i = 0; i < 4; ++i) p->o_mtmp[i] = cv.take((int64_t)B * (D[3] > D[2] ? D[3] : D[2]) * 4);
        // dlogits in storage type: every task's [B, ld_t] block at its logits offset (one cast for all heads; the heads' weight gradients
        // read their blocks from the weight-gradient stream while the data gradient runs)
        p->o_dlT = cv.take((p->logits_numel > 8 ? p->logits_numel : 8) * esz);
    }
    if (c.fp8) {
        int64_t mc = 0, mh = 0;
        for (int s = 0; s < 2; ++s) {
            const int64_t M = (int64_t)B * p->Ntok[s];
            if (M * D[2 + s] > mc) mc = M * D[2 + s];
            if (M * c.mlp_hidden[s] > mh) mh = M * c.mlp_hidden[s];
        }
        p->o_a8 = cv.take(mc);
        p->o_a8s = cv.take(mc / 32);
        p->o_h8 = cv.take(mh);
        p->o_h8s = cv.take(mh / 32);
    }
    if (!inf) {
        p->o_lnws = cv.take(p->lnws_floats * 4);
        {   // a postponed LayerNorm backward keeps its column partials until the segment's flush: LN_DEFER_SLOTS regions, each as large as the
            // largest launch-stream LayerNorm of this plan wants (workgroups x 2C floats; the kernel caps its grid by the region it is given)
            const int64_t rows[5] = {(int64_t)B * p->HW[0], (int64_t)B * p->HW[1], (int64_t)B * p->Ntok[0], (int64_t)B * p->Ntok[1], (int64_t)B};
            const int64_t wide[5] = {D[0], D[1], D[2], D[3], D[3]};
            int64_t need = 0;
            for (int i = 0; i < 5; ++i) {
                int64_t wgs = (rows[i] + 7) / 8;
                if (wgs > 2048) wgs = 2048;
                if (wgs * 2 * wide[i] > need) need = wgs * 2 * wide[i];
            }
            p->lnws_defer_floats = need;
            p->o_lnws_defer = cv.take(need * 4 * LN_DEFER_SLOTS);
        }
        p->o_lnws_side = cv.take(p->lnws_side_floats * 4);
        if (p->det) {
            for (int s = 0; s < 2; ++s) {
                const int M = B * p->HW[s];
                const int64_t dw = lnx_dwconv7_wgrad_ws_floats(B, p->H[s], p->W[s], D[s], LNX_F32, c.dtype), ls = lnx_layerscale_bwd_ws_floats(M, D[s]);
                if (dw > p->detws_floats) p->detws_floats = dw;
                if (ls > p->detws_floats) p->detws_floats = ls;
            }
            p->o_detws = cv.take(p->detws_floats * 4);
        }
        p->o_tnws = cv.take((int64_t)LNX_TN_WS_FLOATS * 4 * TN_WS_SLOTS);
        {   // pwconv2 weight / bias gradient of dY = rs g, before the LayerScale factor (lnx_layerscale_apply_wgrad): [C, 4C] + [C] fp32
            const int64_t cmax = D[0] > D[1] ? D[0] : D[1];
            p->lsws_floats = cmax * 4 * cmax + cmax;
            p->o_lsws = cv.take(p->lsws_floats * 4);
        }  // one region per weight-gradient product of a block (their reduces run as one launch)
        // Fused conv-MLP blocks: the backward materialises act / dH ([M, 4C] each) for the two weight-gradient GEMMs (a
        // recomputing weight-gradient kernel existed in round 2 and was slower: DESIGN.md)
        p->o_sA = cv.take(maxM4C * esz);
        if (any_fused) p->o_sB = cv.take(maxM4C * esz);
        p->o_sC = cv.take(maxMC * esz);
        // (lnx_plan_set_dropout may come after the layout: a training plan always has room for the dropout forward of its RoPE stages)
        p->o_sD = cv.take((maxMC > fwdMC ? maxMC : fwdMC) * esz);
    }
    if (!inf) {
        int64_t gmax = 0, dmax = 0;
        for (int s = 0; s < 2; ++s) {
            if (cut >= p->u_rope[s] + c.rope_depths[s]) continue;  // no block of this stage runs its attention backward
            const int N = p->Ntok[s];
            const int64_t gsz = lnx_attn_bwd_ws_floats_hd(B, N, c.rope_heads[s], D[2 + s] / c.rope_heads[s]) * 4;  // per-workgroup partials of the freqs gradient
            const int64_t dsz = (int64_t)B * c.rope_heads[s] * N * 4;
            if (gsz > gmax) gmax = gsz;
            if (dsz > dmax) dmax = dsz;
        }
        p->gcos_floats = gmax / 4;
        p->o_gcos = cv.take(gmax * FREQ_DEFER_SLOTS);  // one region per attention backward whose freqs fold waits for the segment's flush
        p->o_delta = cv.take(dmax);
    }
    for (int s = 0; s < 2; ++s) {
        const int64_t N = p->Ntok[s], M = B * N, C = D[2 + s], hid = c.mlp_hidden[s];
        for (auto& k : p->rope[s]) {
            k.dm_proj = p->dmask_bytes;
            k.dm_hid = k.dm_proj + M * C;
            k.dm_fc2 = k.dm_hid + M * hid;
            p->dmask_bytes = k.dm_fc2 + M * C;  // M * C and M * hid are multiples of 8: every mask stays 8-byte aligned
            k.dm_attn = p->amask_bytes;
            p->amask_bytes += (int64_t)B * c.rope_heads[s] * N * ((N + 63) / 64 * 64);
        }
    }
    // the image gradient without the fused kernel: dY . W lands here as fp32 [M0, in_chans * 16] before lnx_col2im_stem (stem_w.ld_t != 0: the
    // plan keeps a transposed copy of the stem weight for that product -- apply_cut)
    p->o_dcol = p->want_x && p->stem_w.ld_t ? cv.take((int64_t)B * p->HW[0] * c.in_chans * 16 * 4) : 0;
    p->ws_bytes = cv.cur;
}

extern "C" int lnx_plan_num_units(const lnx_plan* p) { return p ? (int)p->unit_names.size() : 0; }
extern "C" const char* lnx_plan_unit_name(const lnx_plan* p, int u) {
    return (p && u >= 0 && u < (int)p->unit_names.size()) ? p->unit_names[u].c_str() : nullptr;
}
extern "C" int lnx_plan_param_unit(const lnx_plan* p, int i) { return (p && i >= 0 && i < (int)p->unit_of.size()) ? p->unit_of[i] : -1; }
extern "C" int lnx_plan_first_trained_unit(const lnx_plan* p) { return p ? p->cut : -1; }
extern "C" int lnx_plan_last_backward_units(const lnx_plan* p) { return p ? p->bwd_units : -1; }

extern "C" int lnx_plan_set_trainable(lnx_plan* p, const unsigned char* mask) {
    if (!p) FAIL("lnx_plan_set_trainable: null plan");
    if (p->c.inference) FAIL("lnx_plan_set_trainable: this is an inference plan (cfg.inference = 1): it has no backward to cut");
    if (p->bound) FAIL("lnx_plan_set_trainable: the plan is already bound (lnx_plan_bind); the mask changes lnx_plan_workspace_bytes, so set it between create and bind");
    if (!mask) FAIL("lnx_plan_set_trainable: the mask is NULL (one byte per parameter, lnx_plan_num_params of them)");
    int cut = -1;
    for (size_t i = 0; i < p->unit_of.size(); ++i)
        if (mask[i] && (cut < 0 || p->unit_of[i] < cut)) cut = p->unit_of[i];
    if (cut < 0) {
        if (!p->want_x && !p->want_meta)
            FAIL("lnx_plan_set_trainable: the mask is all zero: nothing trains; use an inference plan (cfg.inference = 1) for that, or ask for input gradients first "
                 "(lnx_plan_set_input_grads)");
        cut = (int)p->unit_names.size();  // nothing trains: only the inputs are differentiated
    }
    p->mask_cut = cut;
    apply_cut(p);
    return 0;
}

// The cut the backward stops behind, from the trainable mask and the input-gradient flags, and what depends on it: the transposed copy
// of the stem weight (the image gradient's lnx_gemm_nt, only where lnx_stem_dgrad does not carry the geometry) and the workspace layout.
static void apply_cut(lnx_plan* p) {
    const lnx_mformer_cfg& c = p->c;
    int cut = p->frozen_prefix ? p->mask_cut : 0;  // LNX_FROZEN_PREFIX=0: the full plan, whatever the mask says
    if (p->want_meta && cut > p->u_tok[0]) cut = p->u_tok[0];
    if (p->want_x) cut = 0;
    if (cut >= (int)p->unit_names.size()) cut = p->u_heads;  // (LNX_FROZEN_PREFIX=0 cannot get here; an all-zero mask needs a flag)
    const int ld_t = p->want_x && !lnx_stem_dgrad_ok(c.dtype, c.in_chans, c.img_h, c.img_w, c.dims[0]) ? c.dims[0] : 0;
    if (cut != p->cut || ld_t != p->stem_w.ld_t) {
        p->cut = cut;
        p->stem_w.ld_t = ld_t;
        layout_workspace(p);
    }
}

extern "C" int lnx_plan_set_input_grads(lnx_plan* p, int want_x, int want_meta) {
    if (!p) FAIL("lnx_plan_set_input_grads: null plan");
    if (p->c.inference) FAIL("lnx_plan_set_input_grads: this is an inference plan (cfg.inference = 1): it has no backward");
    if (p->bound) FAIL("lnx_plan_set_input_grads: the plan is already bound (lnx_plan_bind); the flags change lnx_plan_workspace_bytes, so set them between create and bind");
    if (want_meta && p->c.n_meta <= 0) FAIL("lnx_plan_set_input_grads: want_meta on a plan without metadata components (cfg.n_meta = 0)");
    if (!want_x && !want_meta && p->mask_cut >= (int)p->unit_names.size())
        FAIL("lnx_plan_set_input_grads: the trainable mask is all zero, so at least one input gradient must stay wanted");
    p->want_x = want_x != 0;
    p->want_meta = want_meta != 0;
    if (!p->want_x) p->dx_out = nullptr;
    if (!p->want_meta) p->dmeta_out = nullptr;
    apply_cut(p);
    return 0;
}
extern "C" int lnx_plan_input_grads(const lnx_plan* p) { return p ? (p->want_x ? 1 : 0) | (p->want_meta ? 2 : 0) : -1; }
extern "C" int lnx_plan_bind_input_grads(lnx_plan* p, float* dx, float* dmeta) {
    if (!p) FAIL("lnx_plan_bind_input_grads: null plan");
    if (p->c.inference) FAIL("lnx_plan_bind_input_grads: this is an inference plan (cfg.inference = 1): it has no backward");
    if (dx && !p->want_x) FAIL("lnx_plan_bind_input_grads: dx given, but the plan was not asked for the image gradient (lnx_plan_set_input_grads want_x)");
    if (dmeta && !p->want_meta) FAIL("lnx_plan_bind_input_grads: dmeta given, but the plan was not asked for the metadata gradient (lnx_plan_set_input_grads want_meta)");
    if ((((uintptr_t)dx) & 15) != 0 || (((uintptr_t)dmeta) & 3) != 0) FAIL("lnx_plan_bind_input_grads: dx must be 16-byte aligned, dmeta 4-byte aligned");
    p->dx_out = dx;
    p->dmeta_out = dmeta;
    return 0;
}

extern "C" int64_t lnx_plan_dropout_bytes(const lnx_plan* p) { return p ? p->dmask_bytes : 0; }
extern "C" int64_t lnx_plan_attn_dropout_bytes(const lnx_plan* p) { return p ? p->amask_bytes : 0; }

extern "C" int lnx_plan_set_attn_dropout(lnx_plan* p, const unsigned char* masks, float drop_rate) {
    if (!p) FAIL("lnx_plan_set_attn_dropout: null plan");
    if (masks == nullptr || drop_rate == 0.0f) {
        p->amask = nullptr;
        p->a_inv_keep = 1.0f;
        return 0;
    }
    if (!(drop_rate > 0.0f && drop_rate < 1.0f)) FAIL("lnx_plan_set_attn_dropout: drop_rate %g must be in [0, 1)", (double)drop_rate);
    if (p->c.inference) FAIL("lnx_plan_set_attn_dropout: dropout is a training-time operation; this is an inference plan");
    if ((((uintptr_t)masks) & 3) != 0) FAIL("lnx_plan_set_attn_dropout: the mask buffer must be 4-byte aligned");
    p->amask = masks;
    p->a_inv_keep = 1.0f / (1.0f - drop_rate);
    return 0;
}

extern "C" int lnx_plan_set_dropout(lnx_plan* p, const unsigned char* masks, float drop_rate) {
    if (!p) FAIL("lnx_plan_set_dropout: null plan");
    if (masks == nullptr || drop_rate == 0.0f) {
        p->dmask = nullptr;
        p->inv_keep = 1.0f;
        return 0;
    }
    if (!(drop_rate > 0.0f && drop_rate < 1.0f)) FAIL("lnx_plan_set_dropout: drop_rate %g must be in [0, 1)", (double)drop_rate);
    if (p->c.inference) FAIL("lnx_plan_set_dropout: dropout is a training-time operation; this is an inference plan");
    if (p->c.fp8) FAIL("lnx_plan_set_dropout: dropout is not available on fp8 plans");
    if ((((uintptr_t)masks) & 7) != 0) FAIL("lnx_plan_set_dropout: the mask buffer must be 8-byte aligned");
    p->dmask = masks;
    p->inv_keep = 1.0f / (1.0f - drop_rate);
    return 0;
}

// The plans' two extra streams (metadata-head chains; weight-gradient products) exist ONCE per device and process, shared by every plan:
// plans run one after the other on their caller's stream and join everything they forked before they return, and a process with several
// plans (train + eval, bench.py's two legs, one per batch size) would otherwise hold two more streams per plan -- measured with a second plan
// alive: its 256-image step 20.9 ms instead of 19.6 (more streams than hardware queues: a forked stream then shares a queue with the stream it
// forked from and the two serialise, with the fork / join packets on top).  Never destroyed (two streams per device for the process's life).
static hipStream_t shared_stream(int which) {
    static std::mutex mu;
    static hipStream_t tab[2][64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tab[which][dev] && hipStreamCreateWithFlags(&tab[which][dev], hipStreamNonBlocking) != hipSuccess) tab[which][dev] = nullptr;
    return tab[which][dev];
}

extern "C" void lnx_plan_destroy(lnx_plan* p) {
    if (!p) return;
    (void)lnx_gemm_tn_discard();  // no postponed reduce of this thread may outlive the workspace / gradient arena it points into
    (void)lnx_layernorm_bwd_discard();
    if (p->droplists) {
        (void)hipDeviceSynchronize();  // (a kernel of the last step may still read the lists)
        (void)hipFree(p->droplists);
    }
    if (p->side) {
        (void)hipStreamSynchronize(p->side);  // (shared_stream: not destroyed)
        (void)hipEventDestroy(p->ev_fork);
        (void)hipEventDestroy(p->ev_meta);
        for (int i = 0; i < 2; ++i) {
            (void)hipEventDestroy(p->ev_bfork[i]);
            (void)hipEventDestroy(p->ev_bjoin[i]);
        }
    }
    if (p->wgs) {
        (void)hipStreamSynchronize(p->wgs);  // (shared_stream: not destroyed)
        for (int i = 0; i < 4; ++i) {
            (void)hipEventDestroy(p->ev_wf[i]);
            (void)hipEventDestroy(p->ev_wj[i]);
        }
    }
    for (hipEvent_t e : p->ev_pool) (void)hipEventDestroy(e);
    delete p;
}
extern "C" int64_t lnx_plan_workspace_bytes(const lnx_plan* p) { return p ? p->ws_bytes : 0; }
extern "C" int lnx_plan_num_params(const lnx_plan* p) { return p ? (int)p->names.size() : 0; }
extern "C" const char* lnx_plan_param_name(const lnx_plan* p, int i) {
    return (p && i >= 0 && i < (int)p->names.size()) ? p->names[i].c_str() : nullptr;
}
extern "C" int64_t lnx_plan_param_numel(const lnx_plan* p, int i) { return (p && i >= 0 && i < (int)p->numel.size()) ? p->numel[i] : -1; }
extern "C" int lnx_plan_num_drop_calls(const lnx_plan* p) { return p ? p->n_drop : 0; }
extern "C" int64_t lnx_plan_logits_numel(const lnx_plan* p) { return p ? p->logits_numel : 0; }
extern "C" int64_t lnx_plan_logits_offset(const lnx_plan* p, int t) { return (p && t >= 0 && t < p->c.n_tasks) ? p->logit_off[t] : -1; }
extern "C" int lnx_plan_logits_ld(const lnx_plan* p, int t) { return (p && t >= 0 && t < p->c.n_tasks) ? p->logit_ld[t] : -1; }

extern "C" int lnx_plan_bind(lnx_plan* p, const float* const* params, float* const* grads, void* workspace) {
    if (p) p->trunk_valid = false;  // (a new workspace or new parameters: whatever a forward left is not this binding's)
    if (!p || !params || !workspace) FAIL("lnx_plan_bind: null argument");
    {
        // One device per process (one process per GPU): the cached CU count, the per-kernel dynamic-LDS attributes (set once per process) and the
        // two shared side streams belong to the first device a plan is bound on -- a second device would launch with the wrong attributes.
        static std::atomic<int> bound_dev{-1};
        int dev = -1;
        HIPRUN(hipGetDevice(&dev));
        int expect = -1;
        if (!bound_dev.compare_exchange_strong(expect, dev) && expect != dev)
            FAIL("lnx_plan_bind: this process already runs plans on device %d, now device %d is current: the library is one-process-per-GPU", expect, dev);
    }
    const int n = (int)p->names.size();
    p->P.assign(params, params + n);
    for (int i = 0; i < n; ++i)
        if (p->P[i] == nullptr || (((uintptr_t)p->P[i]) & 3) != 0) FAIL("lnx_plan_bind: parameter %s is null or misaligned", p->names[i].c_str());
    p->has_grads = grads != nullptr;
    if (grads) {
        p->G.assign(grads, grads + n);
        for (int i = 0; i < n; ++i)
            if (p->G[i] == nullptr) FAIL("lnx_plan_bind: gradient of %s is null", p->names[i].c_str());
    } else {
        p->G.assign(n, nullptr);
    }
    p->ws = reinterpret_cast<unsigned char*>(workspace);
    if ((((uintptr_t)p->ws) & 255) != 0) FAIL("lnx_plan_bind: workspace must be 256-byte aligned");
    // operand arena starts zeroed: K / N padding stays zero across refreshes
    HIPRUN(hipMemset(p->ws, 0, (size_t)p->arena_end));
    // descriptor tables: [T-typed weights + depthwise taps][fp32-typed weights]
    std::vector<lnx_prep_desc> d;
    int blk = 0;
    auto push_w = [&](OpW* w) {
        lnx_prep_desc e;
        memset(&e, 0, sizeof e);
        e.src = p->P[w->param];
        e.dst = p->ws + w->off;
        e.dst_t = w->ld_t ? p->ws + w->off_t : nullptr;
        e.rows = w->N;
        e.cols = w->K;
        e.ld = w->ld;
        e.ld_t = w->ld_t;
        e.P = w->P;
        e.mode = w->mode;
        e.block_start = blk;
        blk += lnx_prep_blocks(e.rows, e.ld, e.cols, e.ld_t, e.dst_t != nullptr);
        d.push_back(e);
    };
    const bool split = p->esz == 2;  // in fp32 mode everything goes through one fp32 table
    for (OpW* w : p->all_w)
        if (!split || !w->f32) push_w(w);
    for (int s = 0; s < 2; ++s)
        for (auto& k : p->conv[s]) {
            lnx_prep_desc e;
            memset(&e, 0, sizeof e);
            e.src = p->P[k.dww];
            e.dst = p->ws + k.w49;
            e.rows = p->c.dims[s];
            e.cols = 49;
            e.ld = 49;
            e.mode = LNX_PREP_DW49;
            e.block_start = blk;
            blk += lnx_prep_blocks(e.rows, e.ld, e.cols, 0, 0);
            d.push_back(e);
        }
    p->n_descs_t = (int64_t)d.size();
    p->prep_blocks = blk;
    blk = 0;
    if (split)
        for (OpW* w : p->all_w)
            if (w->f32) push_w(w);
    p->n_descs_f = (int64_t)d.size() - p->n_descs_t;
    p->prep_blocks_f = blk;
    if (env_set("LNX_NO_SIDE_STREAM")) p->meta_mode = 0;
    if (const char* e = getenv("LNX_META_STREAM")) p->meta_mode = atoi(e) < 0 || atoi(e) > 2 ? 1 : atoi(e);
    if (p->side == nullptr && p->c.n_meta > 0 && !env_set("LNX_NO_SIDE_STREAM")) {
        p->side = shared_stream(0);
        if (!p->side) FAIL("lnx_plan: no side stream");
        HIPRUN(hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming));
        HIPRUN(hipEventCreateWithFlags(&p->ev_meta, hipEventDisableTiming));
        for (int i = 0; i < 2; ++i) {
            HIPRUN(hipEventCreateWithFlags(&p->ev_bfork[i], hipEventDisableTiming));
            HIPRUN(hipEventCreateWithFlags(&p->ev_bjoin[i], hipEventDisableTiming));
        }
    }
    if (p->wgs == nullptr && !env_off("LNX_WGRAD_STREAM")) {
        p->wgs = shared_stream(1);
        if (!p->wgs) FAIL("lnx_plan: no weight-gradient stream");
        for (int i = 0; i < 4; ++i) {
            HIPRUN(hipEventCreateWithFlags(&p->ev_wf[i], hipEventDisableTiming));
            HIPRUN(hipEventCreateWithFlags(&p->ev_wj[i], hipEventDisableTiming));
        }
    }
    HIPRUN(hipMemcpy(p->ws + p->o_descs, d.data(), d.size() * sizeof(lnx_prep_desc), hipMemcpyHostToDevice));
    HIPRUN(hipDeviceSynchronize());
    p->bound = true;
    p->fwd_done = false;
    return 0;
}
extern "C" int lnx_plan_trunk_valid(const lnx_plan* p) { return p && p->bound && p->trunk_valid ? 1 : 0; }

// ------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------
namespace {

// the stream the metadata heads run on beside the launch stream, nullptr = on the launch stream itself (lnx_plan_set_meta_stream)
hipStream_t meta_stream(const lnx_plan* p) {
    if (p->c.n_meta <= 0 || p->meta_mode == 0) return nullptr;
    // the weight-gradient stream only carries the one-launch chain: the launch-by-launch chain shares scratch with the launch stream's kernels
    // unless it runs on `side` (ln_bwd / wgrad_to below)
    if (p->meta_mode == 2 && p->chain_ok[0] && p->chain_ok[1] && p->wgs != nullptr) return p->wgs;
    return p->side;
}

struct Ctx {
    lnx_plan* p;
    void* st;
    int dt;
    template <typename U> U* at(int64_t off) const { return p->at<U>(off); }
    const void* wptr(const OpW& w) const { return p->ws + w.off; }
    const void* wtptr(const OpW& w) const { return p->ws + w.off_t; }
};

// kernel classes for the profile: 0 gemm_nt, 1 gemm_tn, 2 attention fwd, 3 attention bwd, 4 dwconv (fwd/dgrad), 5 dwconv wgrad
hipEvent_t take_event(lnx_plan* p) {
    if (p->ev_used == p->ev_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        p->ev_pool.push_back(e);
    }
    return p->ev_pool[p->ev_used++];
}
struct Timed {
    lnx_plan* p;
    hipStream_t st;
    bool on;
    lnx_plan::Span sp;
    // classes 0-7: one launch (lnx_plan_profile_begin); classes 8 / 9: a whole block (lnx_plan_profile_begin_spans)
    Timed(const Ctx& c, int cls, double work, double bytes = 0.0)
        : p(c.p), st((hipStream_t)c.st), on(cls >= 0 && (cls >= 8 ? c.p->profile_spans : (c.p->profile && !c.p->profile_spans))) {
        if (on) {
            sp.cls = cls;
            sp.work = work;
            sp.bytes = bytes;
            sp.e0 = take_event(p);
            sp.e1 = take_event(p);
            (void)hipEventRecord(sp.e0, st);
        }
    }
    ~Timed() {
        if (on) {
            (void)hipEventRecord(sp.e1, st);
            p->spans.push_back(sp);
        }
    }
};
// algorithmic HBM bytes of one NT product: each operand read once, each output written once, the fp32 residual read once
double nt_bytes(const Ctx& c, const lnx_gemm_args* a, int a_elem = 0) {
    const double e = c.p->esz, ea = a_elem ? a_elem : e, mn = (double)a->M * a->N;
    return ea * ((double)a->M * a->K + (double)a->N * a->K) + (a->out_f32 ? 4.0 : e) * mn + (a->c2 ? e * mn : 0.0) + (a->aux ? e * mn : 0.0) +
           (a->res ? 4.0 * mn : 0.0) + (a->c8 ? mn * (1.0 + 1.0 / 32) : 0.0);
}
int gemm_nt_t(const Ctx& c, const lnx_gemm_args* a) {
    // profile classes 0/1 are the bulk GEMMs; the M = batch problems of the metadata heads and the tail (another
    // kernel, partly on the side stream) are not counted
    Timed t(c, a->M >= 1024 ? 0 : -1, 2.0 * a->M * a->N * a->K, nt_bytes(c, a));
    return lnx_gemm_nt(a, c.st);
}

// The classification heads' products (M = batch rows): every head in one launch (lnx_gemm_nt_group) where the list qualifies -- bf16 plans --
// otherwise one launch per head.  accumulate: C = res + sum_t A_t . W_t^T (the data gradient wrt the features); hg[0] carries C / res.
int heads_nt(const Ctx& c, lnx_gemm_args* hg, int n, bool accumulate) {
    static const bool off = env_off("LNX_HEADS_GROUP");  // A/B switch
    // a model with more heads than one launch carries goes in several groups; LNX_HEADS_GROUP_MAX (read per call: the tests flip it) makes
    // the groups smaller so that a 4-head fixture walks that path too
    int gmax = LNX_GEMM_GROUP_MAX;
    if (const char* e = getenv("LNX_HEADS_GROUP_MAX")) {
        const int v = atoi(e);
        if (v >= 1 && v < gmax) gmax = v;
    }
    for (int t0 = 0; t0 < n; t0 += gmax) {
        const int m = n - t0 < gmax ? n - t0 : gmax;
        lnx_gemm_args* g = hg + t0;
        if (accumulate && t0 > 0) {  // a second group adds onto what the first one wrote
            g[0].C = hg[0].C; g[0].ldc = hg[0].ldc; g[0].res = (const float*)hg[0].C; g[0].ldres = hg[0].ldc;
        }
        if (!off && lnx_gemm_nt_group_ok(g, m, accumulate ? 1 : 0)) {
            RUN(lnx_gemm_nt_group(g, m, accumulate ? 1 : 0, c.st));
            continue;
        }
        for (int t = 0; t < m; ++t) {
            lnx_gemm_args a = g[t];
            if (accumulate && t > 0) {
                a.C = g[0].C; a.ldc = g[0].ldc; a.res = (const float*)g[0].C; a.ldres = g[0].ldc;
            }
            RUN(gemm_nt_t(c, &a));
        }
    }
    return 0;
}

lnx_gemm_args gemm_base(const Ctx& c, int M, int N, int K, const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, bool out_f32) {
    lnx_gemm_args a;
    memset(&a, 0, sizeof a);
    a.dtype = c.dt;
    a.M = M;
    a.N = N;
    a.K = K;
    a.A = A;
    a.lda = lda;
    a.W = W;
    a.ldw = ldw;
    a.C = C;
    a.ldc = ldc;
    a.out_f32 = out_f32 ? 1 : 0;
    return a;
}

// The compaction list of one branch (all NULL: the branch runs on full rows) and rows per sample
struct Compact {
    const int* nkeep = nullptr;
    const int* m_dev = nullptr;
    const int* perm = nullptr;
    const int* inv = nullptr;
    int rps = 0;
    explicit operator bool() const { return perm != nullptr; }
};

int ln_fwd(const Ctx& c, int M, int C, float eps, const void* x, int xdt, int64_t ldx, lnx_rowmap xm, int wi, int bi, void* y, int ydt, int64_t ldy,
           lnx_rowmap ym, const void* add, int64_t ldadd, float* mean, float* rstd, void* y8 = nullptr, void* y8s = nullptr, Compact cl = Compact()) {
    lnx_ln_args a;
    memset(&a, 0, sizeof a);
    a.perm = cl.perm; a.m_dev = cl.m_dev; a.rows_per_sample = cl.rps;
    a.y8 = y8; a.ldy8 = C; a.y8_scales = y8s;
    a.M = M; a.C = C; a.eps = eps;
    a.x = x; a.x_dtype = xdt; a.ldx = ldx; a.x_map = xm;
    a.w = c.p->P[wi]; a.b = c.p->P[bi];
    a.y = y; a.y_dtype = ydt; a.ldy = ldy; a.y_map = ym;
    a.add = add; a.ldadd = ldadd; a.mean = mean; a.rstd = rstd;
    return lnx_layernorm_fwd(&a, c.st);
}

// A LayerNorm backward whose column-sum reduce waits for the segment's flush (ln_flush below) keeps its partial sums in a region of its
// own until then: takes the next of the LN_DEFER_SLOTS regions, flushing first when all are in use
int ln_defer_slot(const Ctx& c, float*& ws, int64_t& ws_floats) {
    lnx_plan* p = c.p;
    if (p->ln_pending == LN_DEFER_SLOTS) {
        RUN(lnx_layernorm_bwd_flush(c.st));
        p->ln_pending = 0;
    }
    ws = c.at<float>(p->o_lnws_defer) + (int64_t)p->ln_pending * p->lnws_defer_floats;
    ws_floats = p->lnws_defer_floats;
    ++p->ln_pending;
    return 0;
}

// dx2 (optional): DropPath-scaled copy of dx in storage type = the dY operand of the next branch's GEMMs
struct Dx2 {
    void* p = nullptr;
    const float* rowscale = nullptr;
    int rps = 0;
    void* p8 = nullptr;   // fp8 plans with MXFP8 data gradients: the MXFP8 copy of p (elements, block scales), written by the same pass
    void* p8s = nullptr;
    const int* inv = nullptr;    // the branch that reads p runs on compact rows: sample -> position under its list, and its kept count
    const int* nkeep = nullptr;
};
int ln_bwd(const Ctx& c, int M, int C, const void* dy, int dydt, int64_t lddy, lnx_rowmap dym, const void* x, int xdt, int64_t ldx, lnx_rowmap xm, int wi,
           int bi, const float* mean, const float* rstd, const float* gin, void* dx, int dxdt, int64_t lddx, bool relu, Dx2 d2 = Dx2(), Compact cl = Compact()) {
    lnx_ln_bwd_args a;
    memset(&a, 0, sizeof a);
    a.perm = cl.perm; a.m_dev = cl.m_dev; a.dx2_inv = d2.inv; a.dx2_nkeep = d2.nkeep;
    a.dx2 = d2.p; a.dx2_dtype = c.dt; a.lddx2 = C; a.dx2_rowscale = d2.rowscale; a.dx2_rows_per_sample = d2.rps > 0 ? d2.rps : cl.rps;
    if (d2.p && d2.p8) {
        a.dx2_8 = d2.p8; a.dx2_8_scales = d2.p8s; a.lddx2_8 = C;
    }
    a.M = M; a.C = C;
    a.dy = dy; a.dy_dtype = dydt; a.lddy = lddy; a.dy_map = dym;
    a.x = x; a.x_dtype = xdt; a.ldx = ldx; a.x_map = xm;
    a.w = c.p->P[wi]; a.mean = mean; a.rstd = rstd;
    a.gin = gin; a.ldgin = lddx;
    a.dx = dx; a.dx_dtype = dxdt; a.lddx = lddx;
    a.dw = c.p->G[wi]; a.db = c.p->G[bi];
    a.relu_mask = relu ? 1 : 0;
    // the side stream gets its own partial-sum scratch (both streams run LayerNorm backward concurrently)
    const bool on_side = c.p->side != nullptr && c.st == (void*)c.p->side;
    a.ws = c.at<float>(on_side ? c.p->o_lnws_side : c.p->o_lnws);
    a.ws_floats = on_side ? c.p->lnws_side_floats : c.p->lnws_floats;
    // Launch-stream calls postpone their column-sum reduce to the segment's flush.  22 reduce launches of ~8 us per step become 4.
    lnx_plan* p = c.p;
    const bool on_wgs = p->wgs != nullptr && c.st == (void*)p->wgs;  // (the launch stream may be the null stream: compare only with streams that exist)
    if (p->ln_defer && !on_side && !on_wgs && p->o_lnws_defer != 0 && (a.dw || a.db)) {
        RUN(ln_defer_slot(c, a.ws, a.ws_floats));
        a.defer = 1;
    }
    return lnx_layernorm_bwd(&a, c.st);
}

// `slot` >= 0: the product's split-K partial tiles go to workspace region `slot` and their summation into the gradient is postponed to
// the block's tn_flush() (lnx_wgrad_args.defer); -1: summed at once
int wgrad_to(const Ctx& c, int M, int N, int K, const void* dY, int64_t lddy, const void* A, int64_t lda, float* dW, float* db, int64_t lddw, int k_store, int slot,
             const int* m_dev = nullptr) {
    lnx_wgrad_args a;
    memset(&a, 0, sizeof a);
    a.m_dev = m_dev;
    a.dtype = c.dt;
    a.M = M; a.N = N; a.K = K;
    a.dY = dY; a.lddy = lddy;
    a.A = A; a.lda = lda;
    a.dW = dW; a.lddw = lddw;
    a.db = db;
    a.k_store = k_store;
    if (!(c.p->side != nullptr && c.st == (void*)c.p->side)) {  // one workspace: never from the side stream
        a.ws = c.at<float>(c.p->o_tnws) + (int64_t)(slot > 0 ? slot : 0) * LNX_TN_WS_FLOATS;
        a.ws_floats = LNX_TN_WS_FLOATS;
        a.defer = slot >= 0 ? 1 : 0;
    }
    Timed t(c, M >= 1024 ? 1 : -1, 2.0 * M * N * K, (double)c.p->esz * ((double)M * N + (double)M * K) + 8.0 * N * K);
    return lnx_gemm_tn(&a, c.st);
}
// ... into the gradient arena's slices of parameters `wparam` / `bparam`
int wgrad(const Ctx& c, int M, int N, int K, const void* dY, int64_t lddy, const void* A, int64_t lda, int wparam, int bparam, int64_t lddw, int k_store = 0,
          int slot = -1, const int* m_dev = nullptr) {
    return wgrad_to(c, M, N, K, dY, lddy, A, lda, c.p->G[wparam], bparam >= 0 ? c.p->G[bparam] : nullptr, lddw, k_store, slot, m_dev);
}
// ... into explicit buffers (the z-free LayerScale path's scratch)
int wgrad_into(const Ctx& c, int M, int N, int K, const void* dY, int64_t lddy, const void* A, int64_t lda, float* dW, float* db, int64_t lddw, int slot,
               const int* m_dev = nullptr) {
    return wgrad_to(c, M, N, K, dY, lddy, A, lda, dW, db, lddw, 0, slot, m_dev);
}

const lnx_rowmap IDM = {0, 0, 0};

// A RoPE-block Linear in the forward.  On fp8 plans (and M >= 256, the MXFP8 kernel's floor) the product runs on
// lnx_gemm_nt_mxfp8 with the weight's MXFP8 copy and the MXFP8 copy of the activation its producer wrote (`a8` / `a8s`: the
// LayerNorm forward for qkv and fc1, the fc1 epilogue for fc2); `out8` / `out8s` ask this product's epilogue for the MXFP8
// copy of its own output.  The epilogue (bias, GELU + pre-activation copy, fp32 residual with DropPath scale) is the same
// code either way.
// `width` = the narrower side of the block's products (its channel count C: K of qkv / fc1, N of proj / fc2): the MXFP8 kernel
// needs K >= 256 as well as M >= 256, and a block is all-fp8 or all-bf16 because the producers of one product's operand copy
// (LayerNorm, the fc1 epilogue) must match the consumer's choice.
bool fp8_rows(const lnx_plan* p, int M, int width) { return p->c.fp8 != 0 && M >= 256 && width >= 256; }
int linear_fwd(const Ctx& c, lnx_gemm_args g, const OpW& w, int64_t a8, int64_t a8s, int64_t out8 = 0, int64_t out8s = 0) {
    lnx_plan* p = c.p;
    if (!fp8_rows(p, g.M, g.K < g.N ? g.K : g.N) || w.off8s == 0) return gemm_nt_t(c, &g);
    g.A = c.at<void>(a8);
    g.lda = g.K;
    g.W = c.at<void>(w.off8);
    g.ldw = w.K;
    if (out8s) {
        g.c8 = c.at<void>(out8); g.ldc8 = g.N; g.c8_scales = c.at<void>(out8s);
    }
    Timed t(c, g.M >= 1024 ? 0 : -1, 2.0 * g.M * g.N * g.K, nt_bytes(c, &g, 1));
    return lnx_gemm_nt_mxfp8(&g, c.at<void>(a8s), c.at<void>(w.off8s), c.st);
}

// The data-gradient product dX = dY . W of a RoPE-block Linear (NT form on the transposed weight).  fp8 plans: dY comes as
// MXFP8 (`a8` / `a8s`; quantised here from the bf16 `g.A` when `quantise` is set), the weight as its transposed MXFP8 copy.
int linear_dgrad(const Ctx& c, lnx_gemm_args g, const OpW& w, bool quantise, int64_t a8, int64_t a8s, int64_t out8 = 0, int64_t out8s = 0) {
    lnx_plan* p = c.p;
    if (!fp8_rows(p, g.M, g.K < g.N ? g.K : g.N) || w.off8ts == 0) return gemm_nt_t(c, &g);
    if (quantise) RUN(lnx_quantize_mxfp8(g.A, LNX_BF16, g.lda, g.M, g.K, c.at<void>(a8), g.K, c.at<void>(a8s), c.st));
    g.A = c.at<void>(a8);
    g.lda = g.K;
    g.W = c.at<void>(w.off8t);
    g.ldw = w.N;
    if (out8s) {
        g.c8 = c.at<void>(out8); g.ldc8 = g.N; g.c8_scales = c.at<void>(out8s);
    }
    Timed t(c, g.M >= 1024 ? 0 : -1, 2.0 * g.M * g.N * g.K, nt_bytes(c, &g, 1));
    return lnx_gemm_nt_mxfp8(&g, c.at<void>(a8s), c.at<void>(w.off8ts), c.st);
}

// ------------------------------ forward pieces ------------------------------
// The compaction list of a conv block's DropPath call, or none: the forward built it (training plan, both switches on, the call has a
// multiplier, no dropout masks) and the block runs fused with the LayerNorm inside.  The conv-MLP kernels and the two pointwise
// weight-gradient products then run on the kept samples' rows (compact: ln / mean / rstd, act, dh, dz); the depthwise kernels walk
// the kept samples of y / dy (natural order) only.
Compact conv_compact_of(const lnx_plan* p, int s, int i) {
    Compact cl;
    const ConvBlk& k = p->conv[s][i];
    const int* list = p->compact_conv_now && k.fused && k.fused_ln ? p->drop_list(p->drop_conv[s][i]) : nullptr;
    if (list == nullptr) return cl;
    cl.nkeep = list; cl.m_dev = list + 1; cl.perm = list + 2; cl.inv = list + 2 + p->c.batch; cl.rps = p->H[s] * p->W[s];
    return cl;
}

int conv_block_fwd(const Ctx& c, int s, int i, float* xout) {
    lnx_plan* p = c.p;
    ConvBlk& k = p->conv[s][i];
    const int B = p->c.batch, H = p->H[s], W = p->W[s], C = p->c.dims[s];
    const int M = B * H * W;
    p->resident[s] = i;
    Timed span(c, 9, 2.0 * M * C * (8.0 * C + 49.0));
    lnx_dwconv_args d;
    memset(&d, 0, sizeof d);
    d.B = B; d.H = H; d.W = W; d.C = C;
    d.x = c.at<float>(k.xin); d.x_dtype = LNX_F32;
    d.w49 = c.at<float>(k.w49); d.bias = p->P[k.dwb];
    d.y = c.at<void>(k.y); d.y_dtype = c.dt;
    const Compact cl = conv_compact_of(p, s, i);  // y of the dropped samples is then neither written here nor read by the conv-MLP kernel
    {
        Timed t(c, 4, (double)M * C * (4 + p->esz));  // bytes: read fp32 x, write T y
        RUN(lnx_dwconv7_fwd_kept(&d, cl.perm, cl.nkeep, c.st));
    }
    if (!k.fused_ln)
        RUN(ln_fwd(c, M, C, 1e-6f, c.at<void>(k.y), c.dt, C, IDM, k.lnw, k.lnb, c.at<void>(k.ln), c.dt, C, IDM, nullptr, 0, c.at<float>(k.mean), c.at<float>(k.rstd)));
    if (k.fused) {
        lnx_convmlp_args f;
        memset(&f, 0, sizeof f);
        f.dtype = c.dt; f.M = M; f.C = C;
        if (k.fused_ln) {  // the kernel normalises y itself; a training plan keeps the normalised rows and the statistics for the backward
            f.y = c.at<void>(k.y); f.ln_w = p->P[k.lnw]; f.ln_b = p->P[k.lnb]; f.ln_eps = 1e-6f;
            if (!p->c.inference) {
                f.ln_out = c.at<void>(k.ln); f.mean = c.at<float>(k.mean); f.rstd = c.at<float>(k.rstd);
            }
        } else {
            f.ln = c.at<void>(k.ln);
        }
        f.w1 = c.wptr(k.w1); f.b1 = p->P[k.b1]; f.w2 = c.wptr(k.w2); f.b2 = p->P[k.b2];
        f.gamma = p->P[k.gamma]; f.rowscale = p->drop_ptr(p->drop_conv[s][i]); f.rows_per_sample = H * W;
        f.x = c.at<float>(k.xin); f.out = xout;
        f.perm = cl.perm; f.m_dev = cl.m_dev;  // (the kernel copies the dropped samples' rows itself)
        if (cl) g_compact_conv_blocks.fetch_add(1, std::memory_order_relaxed);
        Timed t(c, 6, 2.0 * M * C * 4 * C * 2);
        RUN(lnx_convmlp_fwd(&f, c.st));
        return 0;
    }
    lnx_gemm_args g = gemm_base(c, M, 4 * C, C, c.at<void>(k.ln), C, c.wptr(k.w1), k.w1.ld, c.at<void>(k.act), 4 * C, false);
    g.bias = p->P[k.b1]; g.act = LNX_ACT_GELU;
    if (!p->c.inference) {  // the backward's second tensor: GELU'(h), evaluated here once (as in the RoPE blocks' fc1)
        g.act = LNX_ACT_GELU_D;
        g.c2 = c.at<void>(k.hpre); g.ldc2 = 4 * C;
    }
    RUN(gemm_nt_t(c, &g));
    g = gemm_base(c, M, C, 4 * C, c.at<void>(k.act), 4 * C, c.wptr(k.w2), k.w2.ld, xout, C, true);
    g.bias = p->P[k.b2]; g.c2 = c.at<void>(k.z); g.ldc2 = C;
    g.gamma = p->P[k.gamma]; g.rowscale = p->drop_ptr(p->drop_conv[s][i]); g.rows_per_sample = H * W;
    g.res = c.at<float>(k.xin); g.ldres = C;
    RUN(gemm_nt_t(c, &g));
    return 0;
}

int downsample_fwd(const Ctx& c, int i, const void* x, int xdt, int64_t ldx, lnx_rowmap xm, float* out, int64_t ldout, lnx_rowmap om) {
    lnx_plan* p = c.p;
    Down& d = p->down[i];
    const int B = p->c.batch, Hin = p->H[i], Win = p->W[i], Cin = p->c.dims[i], Cout = p->c.dims[i + 1];
    const int Min = B * Hin * Win, Mout = Min / 4;
    RUN(ln_fwd(c, Min, Cin, 1e-6f, x, xdt, ldx, xm, d.lnw, d.lnb, c.at<void>(d.ln), c.dt, Cin, IDM, nullptr, 0, c.at<float>(d.mean), c.at<float>(d.rstd)));
    lnx_gemm_args g = gemm_base(c, Mout, Cout, 4 * Cin, c.at<void>(d.ln), 0, c.wptr(d.w), d.w.ld, out, ldout, true);
    g.a_mode = LNX_ADDR_PATCH2; g.Hin = Hin; g.Win = Win; g.Cin = Cin;
    g.bias = p->P[d.cb]; g.c_map = om;
    RUN(gemm_nt_t(c, &g));
    return 0;
}

int meta_head_fwd(const Ctx& cc, int s, int m, const float* meta, int meta_width) {
    const Ctx c{cc.p, cc.st, LNX_F32};  // fp32 storage for the M = batch meta-head chain
    lnx_plan* p = c.p;
    MetaHead& k = p->meta[s][m];
    const int B = p->c.batch, C = p->c.dims[2 + s], N = p->Ntok[s];
    float* tok = c.at<float>(p->o_tok[s]);
    RUN(lnx_pack_meta(meta, meta_width, k.off, k.dim, c.at<void>(k.t0), c.dt, B, c.st));
    lnx_gemm_args g = gemm_base(c, B, C, 16, c.at<void>(k.t0), 16, c.wptr(k.w0), k.w0.ld, c.at<void>(k.h0), C, false);
    g.bias = p->P[k.b0]; g.act = LNX_ACT_RELU;
    RUN(gemm_nt_t(c, &g));
    RUN(ln_fwd(c, B, C, 1e-5f, c.at<void>(k.h0), c.dt, C, IDM, k.lnw0, k.lnb0, c.at<void>(k.x), c.dt, C, IDM, nullptr, 0, c.at<float>(k.m0), c.at<float>(k.r0)));
    g = gemm_base(c, B, C, C, c.at<void>(k.x), C, c.wptr(k.w1), k.w1.ld, c.at<void>(k.h1), C, false);
    g.bias = p->P[k.b1]; g.act = LNX_ACT_RELU;
    RUN(gemm_nt_t(c, &g));
    RUN(ln_fwd(c, B, C, 1e-5f, c.at<void>(k.h1), c.dt, C, IDM, k.nf1w, k.nf1b, c.at<void>(k.n1), c.dt, C, IDM, nullptr, 0, c.at<float>(k.m1), c.at<float>(k.r1)));
    g = gemm_base(c, B, C, C, c.at<void>(k.n1), C, c.wptr(k.w2), k.w2.ld, c.at<void>(k.h2), C, false);
    g.bias = p->P[k.b2]; g.act = LNX_ACT_RELU;
    RUN(gemm_nt_t(c, &g));
    const lnx_rowmap om = {1, N - 1, 1 + m};
    RUN(ln_fwd(c, B, C, 1e-5f, c.at<void>(k.h2), c.dt, C, IDM, k.nf2w, k.nf2b, tok, LNX_F32, C, om, c.at<void>(k.x), C, c.at<float>(k.m2), c.at<float>(k.r2)));
    return 0;
}

// All metadata heads of the given stages in one launch (metahead.hip): the chain meta_head_fwd spells out launch by launch
int meta_chain_fwd(const Ctx& c, int s_lo, int s_hi, const float* meta, int meta_width) {
    lnx_plan* p = c.p;
    lnx_meta_head_args a[2 * LNX_MAX_META];
    int n = 0;
    for (int s = s_lo; s < s_hi; ++s)
        for (int m = 0; m < p->c.n_meta; ++m) {
            MetaHead& k = p->meta[s][m];
            const int C = p->c.dims[2 + s], N = p->Ntok[s];
            lnx_meta_head_args& h = a[n++];
            memset(&h, 0, sizeof h);
            h.B = p->c.batch; h.C = C; h.dim = k.dim; h.off = k.off; h.meta = meta; h.meta_width = meta_width; h.eps = 1e-5f;
            h.w0 = (const float*)c.wptr(k.w0); h.ldw0 = k.w0.ld; h.b0 = p->P[k.b0]; h.ln0_w = p->P[k.lnw0]; h.ln0_b = p->P[k.lnb0];
            h.w1 = (const float*)c.wptr(k.w1); h.ldw1 = k.w1.ld; h.b1 = p->P[k.b1]; h.ln1_w = p->P[k.nf1w]; h.ln1_b = p->P[k.nf1b];
            h.w2 = (const float*)c.wptr(k.w2); h.ldw2 = k.w2.ld; h.b2 = p->P[k.b2]; h.ln2_w = p->P[k.nf2w]; h.ln2_b = p->P[k.nf2b];
            h.t0 = c.at<float>(k.t0); h.h0 = c.at<float>(k.h0); h.x = c.at<float>(k.x); h.h1 = c.at<float>(k.h1); h.n1 = c.at<float>(k.n1); h.h2 = c.at<float>(k.h2);
            h.m0 = c.at<float>(k.m0); h.r0 = c.at<float>(k.r0); h.m1 = c.at<float>(k.m1); h.r1 = c.at<float>(k.r1); h.m2 = c.at<float>(k.m2); h.r2 = c.at<float>(k.r2);
            h.tok = c.at<float>(p->o_tok[s]); h.tok_row_stride = (int64_t)N * C; h.tok_row_offset = (int64_t)(1 + m) * C;
        }
    return n ? lnx_meta_heads_fwd(a, n, c.st) : 0;
}

// The metadata gradient (want_meta plans, lnx_meta_input_grad): head m of stage s contributes dp0 . w0 to its component's columns.  A
// component has two heads, one per RoPE stage, and both stages' head backwards run on one stream (meta_stream, or the launch stream) in
// the order stage 4, stage 3: the stage-4 heads WRITE dmeta (every column belongs to a component), the stage-3 heads ADD to it -- a fixed
// order with no atomics and nothing to pre-zero.  Final once the stage-3 heads are joined (the end of segment 2).
int meta_width_of(const lnx_plan* p) {
    int w = 0;
    for (int m = 0; m < p->c.n_meta; ++m) w += p->c.meta_dims[m];
    return w;
}
int meta_accumulates(int s) { return s == 0 ? 1 : 0; }
lnx_meta_input_grad_args meta_input_grad_of(const Ctx& c, int s, int m, const float* dp0) {
    const MetaHead& k = c.p->meta[s][m];
    lnx_meta_input_grad_args a;
    memset(&a, 0, sizeof a);
    a.B = c.p->c.batch; a.C = c.p->c.dims[2 + s]; a.dim = k.dim; a.off = k.off;
    a.dp0 = dp0; a.lddp0 = a.C;
    a.w0 = (const float*)c.wptr(k.w0); a.ldw0 = k.w0.ld;
    return a;
}

// ... and their backward for one stage: g = gradient of the stage's token matrix [B N, C]
int meta_chain_bwd(const Ctx& c, int s, const float* g) {
    lnx_plan* p = c.p;
    lnx_meta_head_bwd_args a[LNX_MAX_META];
    const int C = p->c.dims[2 + s], N = p->Ntok[s];
    for (int m = 0; m < p->c.n_meta; ++m) {
        MetaHead& k = p->meta[s][m];
        lnx_meta_head_bwd_args& h = a[m];
        memset(&h, 0, sizeof h);
        h.B = p->c.batch; h.C = C; h.dim = k.dim;
        h.g = g; h.g_row_stride = (int64_t)N * C; h.g_row_offset = (int64_t)(1 + m) * C;
        h.w1t = (const float*)c.wtptr(k.w1); h.ldw1t = k.w1.ld_t; h.w2t = (const float*)c.wtptr(k.w2); h.ldw2t = k.w2.ld_t;
        h.ln0_w = p->P[k.lnw0]; h.ln1_w = p->P[k.nf1w]; h.ln2_w = p->P[k.nf2w];
        h.t0 = c.at<float>(k.t0); h.h0 = c.at<float>(k.h0); h.x = c.at<float>(k.x); h.h1 = c.at<float>(k.h1); h.n1 = c.at<float>(k.n1); h.h2 = c.at<float>(k.h2);
        h.m0 = c.at<float>(k.m0); h.r0 = c.at<float>(k.r0); h.m1 = c.at<float>(k.m1); h.r1 = c.at<float>(k.r1); h.m2 = c.at<float>(k.m2); h.r2 = c.at<float>(k.r2);
        h.dp2 = c.at<float>(k.dp2); h.dp1 = c.at<float>(k.dp1); h.dp0 = c.at<float>(k.dp0); h.part = c.at<float>(k.part);
        h.d_w0 = p->G[k.w0.param]; h.d_b0 = p->G[k.b0]; h.d_ln0_w = p->G[k.lnw0]; h.d_ln0_b = p->G[k.lnb0];
        h.d_w1 = p->G[k.w1.param]; h.d_b1 = p->G[k.b1]; h.d_ln1_w = p->G[k.nf1w]; h.d_ln1_b = p->G[k.nf1b];
        h.d_w2 = p->G[k.w2.param]; h.d_b2 = p->G[k.b2]; h.d_ln2_w = p->G[k.nf2w]; h.d_ln2_b = p->G[k.nf2b];
    }
    if (p->c.n_meta == 0) return 0;
    RUN(lnx_meta_heads_bwd(a, p->c.n_meta, c.st));
    if (float* dmeta = p->dmeta_dst()) {  // every head of the stage from the dp0 the chain just left, one launch
        lnx_meta_input_grad_args ig[LNX_MAX_META];
        for (int m = 0; m < p->c.n_meta; ++m) ig[m] = meta_input_grad_of(c, s, m, a[m].dp0);
        RUN(lnx_meta_input_grad(ig, p->c.n_meta, dmeta, meta_width_of(p), meta_accumulates(s), c.st));
    }
    return 0;
}

// The metadata heads of stages [s_lo, s_hi), forward: the one-launch chain where it carries the stage's width (chain_ok), else head by head
int meta_fwd(const Ctx& c, int s_lo, int s_hi, const float* meta, int meta_width) {
    lnx_plan* p = c.p;
    bool all_chain = true;
    for (int s = s_lo; s < s_hi; ++s) all_chain = all_chain && p->chain_ok[s];
    if (all_chain) return meta_chain_fwd(c, s_lo, s_hi, meta, meta_width);  // every head of these stages: one call (a launch per width)
    for (int s = s_lo; s < s_hi; ++s) {
        if (p->chain_ok[s]) {
            RUN(meta_chain_fwd(c, s, s + 1, meta, meta_width));
            continue;
        }
        for (int m = 0; m < p->c.n_meta; ++m) RUN(meta_head_fwd(c, s, m, meta, meta_width));
    }
    return 0;
}

// "next block's input, else the stage output": where block i of a stage writes (i = -1: where the stage reads)
float* conv_out(const lnx_plan* p, int s, int i) {
    return p->at<float>(i + 1 < (int)p->conv[s].size() ? p->conv[s][i + 1].xin : p->o_stage_out[s]);
}
float* rope_out(const lnx_plan* p, int s, int i) {
    return p->at<float>(i + 1 < (int)p->rope[s].size() ? p->rope[s][i + 1].xin : p->o_stage_out[2 + s]);
}

// forward FLOPs of one RoPE2DMHSABlock: qkv + proj + fc1 + fc2 products and the two attention products (SURVEY 8d's count;
// heads * head_dim = C)
double rope_block_flops(int B, int N, int C, int hid) {
    const double M = (double)B * N;
    return 2.0 * M * C * (3.0 * C + C + 2.0 * hid) + 4.0 * B * (double)N * N * C;
}

// The compaction list of a RoPE-block branch, or none: the forward built the lists (training plan, the switch on), the call has a DropPath
// multiplier, the block does not run its products in fp8 and no dropout mask (laid out by full rows) is set.
Compact compact_of(const lnx_plan* p, int call, int M, int C, int N) {
    Compact cl;
    const int* list = p->drop_list(call);
    if (list == nullptr || fp8_rows(p, M, C) || p->dmask || p->amask) return cl;
    cl.nkeep = list; cl.m_dev = list + 1; cl.perm = list + 2; cl.inv = list + 2 + p->c.batch; cl.rps = N;
    return cl;
}

int rope_block_fwd(const Ctx& c, int s, int i, float* xout) {
    lnx_plan* p = c.p;
    RopeBlk& k = p->rope[s][i];
    const int B = p->c.batch, C = p->c.dims[2 + s], heads = p->c.rope_heads[s], hid = p->c.mlp_hidden[s];
    const int N = p->Ntok[s], M = B * N, E = p->E;
    const float* xin = c.at<float>(k.xin);
    // DropPath compaction: a branch whose call has a list runs on the kept samples' rows only (compact rows: n1 / qkvbuf / o / lse,
    // n2 / act / hpre and the LayerNorm statistics); the fp32 stream keeps its layout, the dropped samples' rows of xmid / xout are copies
    // CLS-only (the last stage-4 block, lnx_plan::last_cls): LayerNorm 1, qkv and attention on all rows (compact under the attention
    // call's list like any block's); everything behind the attention on the B CLS rows (the MLP call stays off the lists: its M = B
    // products take the multiplier of the row's own sample)
    const bool lc = p->last_cls(s, i);
    const Compact ca = compact_of(p, p->drop_attn[s][i], M, C, N), cm = lc ? Compact() : compact_of(p, p->drop_mlp[s][i], M, C, N);
    g_compact_branches.fetch_add((ca ? 1 : 0) + (cm ? 1 : 0), std::memory_order_relaxed);
    p->resident[2 + s] = i;
    Timed span(c, 8, rope_block_flops(B, N, C, hid));  // (the nominal count, CLS-only or not: DESIGN 5)
    const bool f8 = fp8_rows(p, M, C);
    void* a8 = f8 ? c.at<void>(p->o_a8) : nullptr;
    void* a8s = f8 ? c.at<void>(p->o_a8s) : nullptr;
    RUN(ln_fwd(c, M, C, 1e-5f, xin, LNX_F32, C, IDM, k.n1w, k.n1b, c.at<void>(k.n1), c.dt, C, IDM, nullptr, 0, c.at<float>(k.mean1), c.at<float>(k.rstd1), a8, a8s, ca));
    lnx_gemm_args g = gemm_base(c, M, 3 * C, C, c.at<void>(k.n1), C, c.wptr(k.qkv), k.qkv.ld, c.at<void>(k.qkvbuf), 3 * C, false);
    g.bias = p->P[k.qkvb]; g.m_dev = ca.m_dev;
    RUN(linear_fwd(c, g, k.qkv, p->o_a8, p->o_a8s));
    lnx_attn_args a;
    memset(&a, 0, sizeof a);
    a.dtype = c.dt; a.B = B; a.N = N; a.E = E; a.heads = heads; a.head_dim = C / heads;
    a.qkv = c.at<void>(k.qkvbuf); a.cos_tab = c.at<float>(k.cos); a.o = c.at<void>(k.o); a.lse = c.at<float>(k.lse);
    if (p->c.rope_mode == LNX_ROPE_ROTATE) {
        a.rope_mode = LNX_ROPE_ROTATE; a.sin_tab = c.at<float>(k.dsin);
    }
    if (p->amask) {
        a.drop_mask = p->amask + k.dm_attn; a.drop_inv_keep = p->a_inv_keep;
    }
    {
        Timed t(c, 2, 4.0 * B * (double)N * N * C);
        RUN(lnx_attn_fwd_compact(&a, ca.nkeep, c.st));
    }
    if (lc) {
        // Row b of every operand below is the CLS row of sample b: row b N of o / xin / xmid / xout through a leading dimension of N C (no
        // gather), row b of n2 / act / hpre / mean2 / rstd2.  The other rows of xmid and xout are never written: nobody reads them.
        // DropPath: the multiplier of the sample itself (rows_per_sample = 1).  With a list for the attention call, o holds compact rows:
        // row j N is the CLS row of sample perm[j], the product covers the kept samples (the list's nkeep as its row count) and writes
        // xmid through perm; the dropped samples' CLS rows of xmid are copies of xin's.  The MLP branch has no list: a dropped sample
        // gets res + 0 . z.
        const int64_t ldt = (int64_t)N * C;
        const lnx_rowmap clsrow = {1, N - 1, 0};
        g_last_cls_blocks.fetch_add(1, std::memory_order_relaxed);
        g = gemm_base(c, B, C, C, c.at<void>(k.o), ldt, c.wptr(k.proj), k.proj.ld, c.at<float>(k.xmid), ldt, true);
        g.bias = p->P[k.projb]; g.rowscale = p->drop_ptr(p->drop_attn[s][i]); g.rows_per_sample = 1; g.res = xin; g.ldres = ldt;
        g.m_dev = ca.nkeep; g.perm = ca.perm;
        RUN(gemm_nt_t(c, &g));
        if (ca) RUN(lnx_copy_dropped_rows(xin, c.at<float>(k.xmid), ldt, ca.perm, ca.nkeep, B, 1, C, c.st));
        RUN(ln_fwd(c, B, C, 1e-5f, c.at<float>(k.xmid), LNX_F32, C, clsrow, k.n2w, k.n2b, c.at<void>(k.n2), c.dt, C, IDM, nullptr, 0, c.at<float>(k.mean2), c.at<float>(k.rstd2)));
        g = gemm_base(c, B, hid, C, c.at<void>(k.n2), C, c.wptr(k.fc1), k.fc1.ld, c.at<void>(k.act), hid, false);
        g.bias = p->P[k.fc1b]; g.act = LNX_ACT_GELU_D; g.c2 = c.at<void>(k.hpre); g.ldc2 = hid;
        if (p->c.inference) {
            g.act = LNX_ACT_GELU; g.c2 = nullptr; g.ldc2 = 0;
        }
        RUN(gemm_nt_t(c, &g));
        g = gemm_base(c, B, C, hid, c.at<void>(k.act), hid, c.wptr(k.fc2), k.fc2.ld, xout, ldt, true);
        g.bias = p->P[k.fc2b]; g.rowscale = p->drop_ptr(p->drop_mlp[s][i]); g.rows_per_sample = 1; g.res = c.at<float>(k.xmid); g.ldres = ldt;
        RUN(gemm_nt_t(c, &g));
        return 0;
    }
    if (p->dmask) {
        // proj_drop (rope_2d_mhsa.py:503): the product with its bias goes to scratch, dropout + DropPath + residual in one pass
        g = gemm_base(c, M, C, C, c.at<void>(k.o), C, c.wptr(k.proj), k.proj.ld, c.at<void>(p->o_sD), C, false);
        g.bias = p->P[k.projb];
        RUN(gemm_nt_t(c, &g));
        RUN(lnx_dropout_residual(c.at<void>(p->o_sD), c.dt, p->dmask + k.dm_proj, p->inv_keep, p->drop_ptr(p->drop_attn[s][i]), N, xin, c.at<float>(k.xmid), M, C, c.st));
    } else {
        g = gemm_base(c, M, C, C, c.at<void>(k.o), C, c.wptr(k.proj), k.proj.ld, c.at<float>(k.xmid), C, true);
        g.bias = p->P[k.projb]; g.rowscale = p->drop_ptr(p->drop_attn[s][i]); g.rows_per_sample = N; g.res = xin; g.ldres = C;
        g.m_dev = ca.m_dev; g.perm = ca.perm;
        RUN(gemm_nt_t(c, &g));
        if (ca) RUN(lnx_copy_dropped_rows(xin, c.at<float>(k.xmid), C, ca.perm, ca.nkeep, B, N, C, c.st));  // x + 0 . branch(x) = x, bit for bit
    }
    RUN(ln_fwd(c, M, C, 1e-5f, c.at<float>(k.xmid), LNX_F32, C, IDM, k.n2w, k.n2b, c.at<void>(k.n2), c.dt, C, IDM, nullptr, 0, c.at<float>(k.mean2), c.at<float>(k.rstd2), a8, a8s, cm));
    g = gemm_base(c, M, hid, C, c.at<void>(k.n2), C, c.wptr(k.fc1), k.fc1.ld, c.at<void>(k.act), hid, false);
    g.m_dev = cm.m_dev;
    // k.hpre holds GELU'(fc1 output) on bf16 / fp32 plans (evaluated here, once, from the fp32 pre-activation: the data-gradient
    // product's epilogue is then one multiply), the pre-activation itself in blocks that run their products in fp8 (those epilogue forms predate this)
    g.bias = p->P[k.fc1b]; g.act = f8 ? LNX_ACT_GELU : LNX_ACT_GELU_D; g.c2 = c.at<void>(k.hpre); g.ldc2 = hid;
    if (p->c.inference && !f8) {  // nobody differentiates an inference plan: one output, no GELU' tensor
        g.act = LNX_ACT_GELU; g.c2 = nullptr; g.ldc2 = 0;
    }
    RUN(linear_fwd(c, g, k.fc1, p->o_a8, p->o_a8s, p->o_h8, p->o_h8s));
    if (p->dmask) {
        // Mlp.drop after the activation and after fc2 (blocks/mlp.py:63,65); the saved `act` is the dropped one, which is
        // what fc2 and its weight gradient consume
        RUN(lnx_dropout_mul(c.at<void>(k.act), c.dt, p->dmask + k.dm_hid, p->inv_keep, M, hid, c.st));
        g = gemm_base(c, M, C, hid, c.at<void>(k.act), hid, c.wptr(k.fc2), k.fc2.ld, c.at<void>(p->o_sD), C, false);
        g.bias = p->P[k.fc2b];
        RUN(gemm_nt_t(c, &g));
        RUN(lnx_dropout_residual(c.at<void>(p->o_sD), c.dt, p->dmask + k.dm_fc2, p->inv_keep, p->drop_ptr(p->drop_mlp[s][i]), N, c.at<float>(k.xmid), xout, M, C, c.st));
        return 0;
    }
    g = gemm_base(c, M, C, hid, c.at<void>(k.act), hid, c.wptr(k.fc2), k.fc2.ld, xout, C, true);
    g.bias = p->P[k.fc2b]; g.rowscale = p->drop_ptr(p->drop_mlp[s][i]); g.rows_per_sample = N; g.res = c.at<float>(k.xmid); g.ldres = C;
    g.m_dev = cm.m_dev; g.perm = cm.perm;
    RUN(linear_fwd(c, g, k.fc2, p->o_h8, p->o_h8s));
    if (cm) RUN(lnx_copy_dropped_rows(c.at<float>(k.xmid), xout, C, cm.perm, cm.nkeep, B, N, C, c.st));
    return 0;
}

int tokens_to_heads(const Ctx& c, const float* meta, int mw_all, hipStream_t mst, float* feats, float* logits);

// lnx_plan_forward without the trunk-validity bookkeeping of its caller below
int plan_forward(lnx_plan* p, const float* x, const float* meta, const float* drop_scales, const unsigned char* drop_mask, float* feats, float* logits,
                 void* stream) {
    if (!p || !p->bound) FAIL("lnx_plan_forward: plan is not bound");
    if (!x) FAIL("lnx_plan_forward: null input");
    const lnx_mformer_cfg& cf = p->c;
    if (cf.n_meta > 0 && !meta) FAIL("lnx_plan_forward: metadata components are configured but meta is NULL");
    if (cf.n_tasks > 0 && !logits) FAIL("lnx_plan_forward: logits buffer is NULL");
    Ctx c{p, stream, cf.dtype};
    const int B = cf.batch;
    const int* D = cf.dims;
    p->last_drop = drop_scales;
    p->mask_host.assign(p->n_drop, 0);
    if (drop_scales && drop_mask)
        for (int i = 0; i < p->n_drop; ++i) p->mask_host[i] = drop_mask[i];
    p->last_meta = meta;

    // 0. refresh the T-typed operand arena from the fp32 master parameters
    RUN(lnx_prep_weights(c.at<lnx_prep_desc>(p->o_descs), (int)p->n_descs_t, (int)p->prep_blocks, cf.dtype, stream));
    if (p->n_descs_f > 0)
        RUN(lnx_prep_weights(c.at<lnx_prep_desc>(p->o_descs) + p->n_descs_t, (int)p->n_descs_f, (int)p->prep_blocks_f, LNX_F32, stream));
    if (cf.fp8)  // MXFP8 copies of the RoPE blocks' forward weights, straight from the fp32 masters
        for (int s = 0; s < 2; ++s)
            for (auto& k : p->rope[s]) {
                for (const OpW* w : {&k.qkv, &k.fc1, &k.fc2})
                    RUN(lnx_quantize_mxfp8(p->P[w->param], LNX_F32, w->K, w->N, w->K, c.at<void>(w->off8), w->K, c.at<void>(w->off8s), stream));
                for (const OpW* w : {&k.proj, &k.fc1, &k.fc2})  // transposed copies for the data-gradient products, from the bf16 arena
                    if (w->off8ts)
                        RUN(lnx_quantize_mxfp8(c.wtptr(*w), LNX_BF16, w->ld_t, w->K, w->N, c.at<void>(w->off8t), w->N, c.at<void>(w->off8ts), stream));
            }

    // DropPath compaction lists of the RoPE blocks' and the fused conv blocks' drop calls of this forward, one launch (the multipliers are
    // drawn on the device: no host synchronisation).  LNX_DROP_COMPACT=0 / lnx_set_drop_compact(0): every branch on full rows, as before;
    // LNX_DROP_COMPACT_CONV=0: the conv blocks alone.
    // CLS-only last block, decided per forward.  LNX_LAST_CLS=0 / lnx_set_last_cls(0): the full block.  Plans the path does not
    // cover keep the full block as well: fp8 plans (their LayerNorm / fc1 epilogues hand MXFP8 copies on by full rows) and plans with
    // dropout masks (DROP_RATE / ATTN_DROP_RATE > 0: the masks are laid out by full rows).
    {
        const int sw = g_last_cls.load(std::memory_order_relaxed);
        const bool on = sw < 0 ? !env_off("LNX_LAST_CLS") : sw != 0;
        p->last_cls_now = on && cf.rope_depths[1] > 0 && cf.fp8 == 0 && !p->dmask && !p->amask;
    }
    p->compact_now = false;
    p->compact_conv_now = false;
    {
        const int sw = g_drop_compact.load(std::memory_order_relaxed);
        const bool on = sw < 0 ? !env_off("LNX_DROP_COMPACT") : sw != 0;
        if (on && !cf.inference && p->n_drop > 0 && drop_scales && !p->dmask && !p->amask) {
            std::vector<unsigned char> want(p->n_drop, 0);
            std::vector<int> rps(p->n_drop, 1);
            bool any = false, any_conv = false;
            if (!env_off("LNX_DROP_COMPACT_CONV"))  // the conv blocks that run fused with the LayerNorm inside (conv_compact_of)
                for (int s = 0; s < 2; ++s)
                    for (size_t i = 0; i < p->conv[s].size(); ++i) {
                        const int call = p->drop_conv[s][i];
                        if (p->mask_host[call] && p->conv[s][i].fused && p->conv[s][i].fused_ln) {
                            want[call] = 1;
                            rps[call] = p->H[s] * p->W[s];
                            any = any_conv = true;
                        }
                    }
            for (int s = 0; s < 2; ++s)
                for (size_t i = 0; i < p->rope[s].size(); ++i)
                    for (const int call : {p->drop_attn[s][i], p->drop_mlp[s][i]})
                        // (the CLS-only block's MLP call stays off the lists: its M = B products take the multiplier of the row's own sample)
                        if (p->mask_host[call] && !fp8_rows(p, B * p->Ntok[s], D[2 + s]) && !(p->last_cls((int)s, (int)i) && call == p->drop_mlp[s][i])) {
                            want[call] = 1;
                            rps[call] = p->Ntok[s];
                            any = true;
                        }
            if (any) {
                if (p->droplists == nullptr) HIPRUN(hipMalloc((void**)&p->droplists, (size_t)p->n_drop * LNX_DROP_LIST_INTS(B) * sizeof(int)));
                RUN(lnx_drop_partition(drop_scales, p->n_drop, B, want.data(), rps.data(), p->droplists, stream));
                p->compact_now = true;
                p->compact_conv_now = any_conv;
            }
        }
    }

    // metadata heads of both RoPE stages: forked onto the side stream right after the weight refresh
    int mw_all = 0;
    for (int m = 0; m < cf.n_meta; ++m) mw_all += cf.meta_dims[m];
    hipStream_t const mst = meta_stream(p);
    if (mst) {
        HIPRUN(hipEventRecord(p->ev_fork, (hipStream_t)stream));
        HIPRUN(hipStreamWaitEvent(mst, p->ev_fork, 0));
        RUN(meta_fwd(Ctx{p, (void*)mst, cf.dtype}, 0, 2, meta, mw_all));
    }
    {   // the cos tables of every RoPE block in one launch (each block owns its freqs); beside the stem and the ConvNeXt stages when there
        // is a side stream, which the RoPE stages join below.  A checkpointed block's re-forward reads the same tables.
        std::vector<lnx_rope_table> tabs;
        for (int s = 0; s < 2; ++s)
            for (auto& k : p->rope[s]) {
                lnx_rope_table t;
                memset(&t, 0, sizeof t);
                t.freqs = p->P[k.freqs]; t.heads = cf.rope_heads[s]; t.H = p->H[2 + s]; t.W = p->W[2 + s]; t.head_dim = cf.dims[2 + s] / cf.rope_heads[s];
                t.cos_out = c.at<float>(k.cos);
                if (cf.rope_mode == LNX_ROPE_ROTATE) {
                    t.rope_mode = LNX_ROPE_ROTATE; t.sin_out = c.at<float>(k.dsin);
                } else {
                    t.dsin_out = cf.inference ? nullptr : c.at<float>(k.dsin);
                }
                tabs.push_back(t);
            }
        if (!tabs.empty()) RUN(lnx_rope_cos_tables(tabs.data(), (int)tabs.size(), mst ? (void*)mst : stream));
    }
    if (mst) HIPRUN(hipEventRecord(p->ev_meta, mst));

    // 1. stem: 4x4/4 patchify conv as im2col + GEMM, then channels-first LN (mFormerV1.py:145-148)
    const int M0 = B * p->HW[0];
    float* first = conv_out(p, 0, -1);
    if (lnx_stem_fwd_ok(cf.dtype, cf.in_chans, cf.img_h, cf.img_w, D[0])) {
        lnx_stem_args sa;
        memset(&sa, 0, sizeof sa);
        sa.x = x; sa.w = c.wptr(p->stem_w); sa.bias = p->P[p->stem_b]; sa.ln_w = p->P[p->stem_lnw]; sa.ln_b = p->P[p->stem_lnb];
        sa.y = first;
        if (!cf.inference) {  // what the backward reads
            sa.patches = c.at<void>(p->o_patches); sa.pre = c.at<void>(p->o_stem_pre);
            sa.mean = c.at<float>(p->o_stem_mean); sa.rstd = c.at<float>(p->o_stem_rstd);
        }
        sa.B = B; sa.Cin = cf.in_chans; sa.H = cf.img_h; sa.W = cf.img_w; sa.Cout = D[0]; sa.eps = 1e-6f;
        RUN(lnx_stem_fwd(&sa, stream));
    } else {
        RUN(lnx_im2col_stem(x, B, cf.in_chans, cf.img_h, cf.img_w, c.at<void>(p->o_patches), cf.dtype, 64, stream));
        {
            lnx_gemm_args g = gemm_base(c, M0, D[0], 64, c.at<void>(p->o_patches), 64, c.wptr(p->stem_w), 64, c.at<void>(p->o_stem_pre), D[0], false);
            g.bias = p->P[p->stem_b];
            RUN(gemm_nt_t(c, &g));
        }
        RUN(ln_fwd(c, M0, D[0], 1e-6f, c.at<void>(p->o_stem_pre), cf.dtype, D[0], IDM, p->stem_lnw, p->stem_lnb, first, LNX_F32, D[0], IDM, nullptr, 0,
                   c.at<float>(p->o_stem_mean), c.at<float>(p->o_stem_rstd)));
    }

    // 2. ConvNeXt stages + downsamplers (mFormerV1.py:427-443)
    for (int s = 0; s < 2; ++s) {
        for (int i = 0; i < cf.conv_depths[s]; ++i) RUN(conv_block_fwd(c, s, i, conv_out(p, s, i)));
        if (s == 0) {
            RUN(downsample_fwd(c, 0, c.at<float>(p->o_stage_out[0]), LNX_F32, D[0], IDM, conv_out(p, 1, -1), D[1], IDM));
        } else {
            const lnx_rowmap tm = {p->HW[2], p->E, p->E};
            RUN(downsample_fwd(c, 1, c.at<float>(p->o_stage_out[1]), LNX_F32, D[1], IDM, c.at<float>(p->o_tok[0]), D[2], tm));
        }
    }

    // 3. RoPE stages, 4. tail and heads
    RUN(tokens_to_heads(c, meta, mw_all, mst, feats, logits));
    p->fwd_done = true;
    return 0;
}

// Sections 3 and 4 of the forward: everything behind the token boundary.  Reads the patch rows of o_tok[0] (downsample 2 wrote them: section 2)
// and the metadata rows of both token buffers; writes the CLS rows, o_tok[1]'s patch rows and every buffer behind them.  The metadata
// rows: with a side stream (mst) the heads were forked there and are joined here; without one they run here, stage by stage; meta == NULL
// (lnx_plan_forward_tail): the caller has already written them on this stream, nothing to run or to join.
int tokens_to_heads(const Ctx& c, const float* meta, int mw_all, hipStream_t mst, float* feats, float* logits) {
    lnx_plan* p = c.p;
    const lnx_mformer_cfg& cf = p->c;
    void* const stream = c.st;
    const int B = cf.batch;
    const int* D = cf.dims;
    // 3. RoPE stages (mFormerV1.py:445-510)
    for (int s = 0; s < 2; ++s) {
        const int N = p->Ntok[s], C = D[2 + s];
        float* tok = c.at<float>(p->o_tok[s]);
        const lnx_rowmap clsmap = {1, N - 1, 0};
        RUN(lnx_fill_rows(p->P[p->cls[s]], tok, C, clsmap, B, C, stream));
        if (meta == nullptr) {
            // (the tail entry point: both stages' metadata rows are already written, in stream order; or a plan without metadata components)
        } else if (mst) {
            if (s == 0) HIPRUN(hipStreamWaitEvent((hipStream_t)stream, p->ev_meta, 0));  // join: all meta tokens written
        } else {
            RUN(meta_fwd(c, s, s + 1, meta, mw_all));
        }
        for (int i = 0; i < cf.rope_depths[s]; ++i) RUN(rope_block_fwd(c, s, i, rope_out(p, s, i)));
        if (s == 0) {
            const int M2 = B * p->Ntok[0];
            // norm_1 over all tokens (mFormerV1.py:470); T output feeds cl_1_fc and downsample 3
            RUN(ln_fwd(c, M2, C, 1e-5f, c.at<float>(p->o_stage_out[2]), LNX_F32, C, IDM, p->norm_w[0], p->norm_b[0], c.at<void>(p->o_t1), cf.dtype, C, IDM,
                       nullptr, 0, c.at<float>(p->o_t1_mean), c.at<float>(p->o_t1_rstd)));
            if (!cf.only_last_cls) {
                // cl_1_fc = Mlp(D2, D2, D3) + LayerNorm on the CLS row (mFormerV1.py:316-321,474-476)
                lnx_gemm_args g = gemm_base(c, B, D[2], D[2], c.at<void>(p->o_t1), (int64_t)p->Ntok[0] * D[2], c.wptr(p->cl_w1), p->cl_w1.ld, c.at<void>(p->o_cl_act),
                                            D[2], false);
                g.bias = p->P[p->cl_b1]; g.act = LNX_ACT_GELU; g.c2 = c.at<void>(p->o_cl_hpre); g.ldc2 = D[2];
                RUN(gemm_nt_t(c, &g));
                g = gemm_base(c, B, D[3], D[2], c.at<void>(p->o_cl_act), D[2], c.wptr(p->cl_w2), p->cl_w2.ld, c.at<float>(p->o_cl_u), D[3], true);
                g.bias = p->P[p->cl_b2];
                RUN(gemm_nt_t(c, &g));
                RUN(ln_fwd(c, B, D[3], 1e-5f, c.at<float>(p->o_cl_u), LNX_F32, D[3], IDM, p->cl_lnw, p->cl_lnb, c.at<float>(p->o_c1n), LNX_F32, D[3], IDM, nullptr,
                           0, c.at<float>(p->o_cl_mean), c.at<float>(p->o_cl_rstd)));
            }
            // patch tokens -> downsample 3 -> stage-4 tokens (mFormerV1.py:479-483)
            const lnx_rowmap pm = {p->HW[2], p->E, p->E};
            const lnx_rowmap tm = {p->HW[3], p->E, p->E};
            RUN(downsample_fwd(c, 2, c.at<void>(p->o_t1), cf.dtype, C, pm, c.at<float>(p->o_tok[1]), D[3], tm));
        }
    }

    // 4. tail: norm_2 on the CLS row, aggregate, final_norm, heads (mFormerV1.py:509-541)
    {
        const int C = D[3];
        const lnx_rowmap clsrow = {1, p->Ntok[1] - 1, 0};
        RUN(ln_fwd(c, B, C, 1e-5f, c.at<float>(p->o_stage_out[3]), LNX_F32, C, clsrow, p->norm_w[1], p->norm_b[1], c.at<float>(p->o_c2n), LNX_F32, C, IDM, nullptr,
                   0, c.at<float>(p->o_n2_mean), c.at<float>(p->o_n2_rstd)));
        const float* fin_in = c.at<float>(p->o_c2n);
        if (!cf.only_last_cls) {
            RUN(lnx_agg2_fwd(c.at<float>(p->o_c1n), c.at<float>(p->o_c2n), p->P[p->agg_w], p->P[p->agg_b], c.at<float>(p->o_agg), B, C, stream));
            fin_in = c.at<float>(p->o_agg);
        }
        RUN(ln_fwd(c, B, C, 1e-5f, fin_in, LNX_F32, C, IDM, p->fin_w, p->fin_b, c.at<float>(p->o_feats), LNX_F32, C, IDM, nullptr, 0, c.at<float>(p->o_fin_mean),
                   c.at<float>(p->o_fin_rstd)));
        if (feats) HIPRUN(hipMemcpyAsync(feats, c.at<float>(p->o_feats), (size_t)B * C * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        if (cf.n_tasks > 0) {
            RUN(lnx_scale_cast(c.at<float>(p->o_feats), C, IDM, nullptr, 0, c.at<void>(p->o_featsT), cf.dtype, C, B, C, stream));
            lnx_gemm_args hg[LNX_MAX_TASKS];
            for (int t = 0; t < cf.n_tasks; ++t) {
                hg[t] = gemm_base(c, B, cf.task_classes[t], C, c.at<void>(p->o_featsT), C, c.wptr(p->head_w[t]), p->head_w[t].ld, logits + p->logit_off[t],
                                  p->logit_ld[t], true);
                hg[t].bias = p->P[p->head_b[t]];
            }
            RUN(heads_nt(c, hg, cf.n_tasks, false));  // every head in one launch where the grouped kernel takes them
        }
    }
    return 0;
}

}  // namespace

extern "C" int lnx_plan_forward(lnx_plan* p, const float* x, const float* meta, const float* drop_scales, const unsigned char* drop_mask, float* feats,
                                float* logits, void* stream) {
    if (p) p->trunk_valid = false;  // a new trunk starts here; it counts once every launch of this call is enqueued
    RUN(plan_forward(p, x, meta, drop_scales, drop_mask, feats, logits, stream));
    p->trunk_valid = p->c.inference != 0;
    return 0;
}

// Metadata variants: the forward again from the token boundary.  The metadata heads of both stages on the caller's stream (no fork, no
// events: there is no trunk to run beside), then sections 3 and 4 as the forward ran them, with the forward's CLS-only decision.
extern "C" int lnx_plan_forward_tail(lnx_plan* p, const float* meta, float* feats, float* logits, void* stream) {
    if (!p) FAIL("lnx_plan_forward_tail: plan is NULL (nothing bound)");
    const bool had_trunk = p->bound && p->trunk_valid;
    p->trunk_valid = false;  // (set again below: every refusal and every failed launch leaves the plan without a trunk)
    const lnx_mformer_cfg& cf = p->c;
    if (!cf.inference) FAIL("lnx_plan_forward_tail: inference plans only: a training plan keeps one set of activations for its backward");
    if (cf.n_meta <= 0) FAIL("lnx_plan_forward_tail: the plan has no metadata components: nothing to vary");
    if (!meta) FAIL("lnx_plan_forward_tail: meta is NULL");
    if (cf.n_tasks > 0 && !logits) FAIL("lnx_plan_forward_tail: logits buffer is NULL");
    if (!p->bound) FAIL("lnx_plan_forward_tail: plan is not bound: no trunk to continue from");
    if (!had_trunk) FAIL("lnx_plan_forward_tail: no valid trunk: call lnx_plan_forward on this plan first (lnx_plan_bind and a failed call discard it)");
    Ctx c{p, stream, cf.dtype};
    int mw_all = 0;
    for (int m = 0; m < cf.n_meta; ++m) mw_all += cf.meta_dims[m];
    p->last_meta = meta;
    RUN(meta_fwd(c, 0, 2, meta, mw_all));
    RUN(tokens_to_heads(c, nullptr, mw_all, nullptr, feats, logits));
    p->trunk_valid = true;
    return 0;
}

// ------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------
namespace {

// have_dy: the caller's last LayerNorm backward already left this block's MLP-branch dY (DropPath-scaled g in storage
// type) in sC; on return sC holds the same for block i-1 (written by this block's norm1 backward), if there is one
// Weight-gradient stream (lnx_plan::wgs): wg_fork(j) = product j may start (its operands are written), wg_done(j) marks its end on that
// stream, wg_join(j) = the main stream goes on only when product j is done (its dY buffer is about to be overwritten, or the block's
// gradients are about to count as written).  Without the stream all three do nothing and wg_ctx() is the caller's own context.
static inline bool wg_on(const lnx_plan* p) { return p->wgs != nullptr && p->wgs_on; }
Ctx wg_ctx(const Ctx& c) { return Ctx{c.p, wg_on(c.p) ? (void*)c.p->wgs : c.st, c.dt}; }
int wg_fork(const Ctx& c, int j) {
    if (!wg_on(c.p)) return 0;
    HIPRUN(hipEventRecord(c.p->ev_wf[j], (hipStream_t)c.st));
    HIPRUN(hipStreamWaitEvent(c.p->wgs, c.p->ev_wf[j], 0));
    return 0;
}
int wg_done(const Ctx& c, int j) {
    if (!wg_on(c.p)) return 0;
    HIPRUN(hipEventRecord(c.p->ev_wj[j], c.p->wgs));
    return 0;
}
int wg_join(const Ctx& c, int j) {
    if (!wg_on(c.p)) return 0;
    HIPRUN(hipStreamWaitEvent((hipStream_t)c.st, c.p->ev_wj[j], 0));
    return 0;
}

int rope_block_bwd(const Ctx& c, int s, int i, float* g, bool have_dy) {
    lnx_plan* p = c.p;
    RopeBlk& k = p->rope[s][i];
    const int B = p->c.batch, C = p->c.dims[2 + s], heads = p->c.rope_heads[s], hid = p->c.mlp_hidden[s];
    const int N = p->Ntok[s], M = B * N, E = p->E;
    void* sA = c.at<void>(p->o_sA);
    void* sC = c.at<void>(p->o_sC);
    void* sD = c.at<void>(p->o_sD);
    Timed span(c, 8, 2.0 * rope_block_flops(B, N, C, hid));
    const Ctx cw = wg_ctx(c);
    auto wfork = [&](int j) { return wg_fork(c, j); };
    auto wdone = [&](int j) { return wg_done(c, j); };
    auto wjoin = [&](int j) { return wg_join(c, j); };
    // DropPath compaction (the forward's decision, from the same lists): sC / sA / sD hold compact rows inside a branch, g keeps its layout
    // CLS-only (the forward's decision, lnx_plan::last_cls): g is zero outside the CLS rows and this block's MLP branch and proj pair saved
    // B rows, so both run on Mb = B rows -- row b is row b N of g / xmid / o (row map, leading dimension), row b of everything else
    const bool lc = p->last_cls(s, i);
    if (lc && have_dy) FAIL("rope_block_bwd: the CLS-only block takes its dY from g, not from a LayerNorm backward above it");
    // The attention call's list holds as for any block (o, sC and sD are compact under it: sample perm[j]'s CLS row is row j N of o and
    // sD, row j of sC, and the proj pair covers nkeep rows); the MLP call has none.
    const int Mb = lc ? B : M, rps = lc ? 1 : N;
    const lnx_rowmap tm = lc ? lnx_rowmap{1, N - 1, 0} : IDM;
    const int64_t ldo = lc ? (int64_t)N * C : C;
    const Compact ca = compact_of(p, p->drop_attn[s][i], M, C, N), cm = lc ? Compact() : compact_of(p, p->drop_mlp[s][i], M, C, N);
    const int* pj_mdev = lc ? ca.nkeep : ca.m_dev;  // effective rows of the proj pair
    const bool prev_runs = i > 0 && p->runs(p->u_rope[s] + i - 1);  // block i - 1 is not behind the cut: it takes its dY from this block's norm1 backward
    const Compact cprev = prev_runs ? compact_of(p, p->drop_mlp[s][i - 1], M, C, N) : Compact();
    // ---- MLP branch ----
    if (!have_dy) {
        if (cm) RUN(lnx_scale_cast_compact(g, C, p->drop_ptr(p->drop_mlp[s][i]), N, cm.perm, cm.m_dev, sC, c.dt, C, M, C, c.st));
        else RUN(lnx_scale_cast(g, C, tm, p->drop_ptr(p->drop_mlp[s][i]), rps, sC, c.dt, C, Mb, C, c.st));
    }
    if (p->dmask) RUN(lnx_dropout_mul(sC, c.dt, p->dmask + k.dm_fc2, p->inv_keep, M, C, c.st));  // through the dropout after fc2
    RUN(wfork(0));
    RUN(wgrad(cw, Mb, C, hid, sC, C, c.at<void>(k.act), hid, k.fc2.param, k.fc2b, hid, 0, 0, cm.m_dev));
    RUN(wdone(0));
    lnx_gemm_args a = gemm_base(c, Mb, hid, C, sC, C, c.wtptr(k.fc2), k.fc2.ld_t, sA, hid, false);
    a.m_dev = cm.m_dev;
    a.act = fp8_rows(p, M, C) ? LNX_ACT_GELU_BWD : LNX_ACT_MUL_AUX; a.aux = c.at<void>(k.hpre); a.ldaux = hid;  // what the forward left in hpre
    // fp8 plans: dY comes in MXFP8 from the LayerNorm backward that wrote it (the block above's norm1 backward; quantised here when
    // there was none, or a dropout mask went over it since), the GELU' epilogue hands dH on in MXFP8 as well as in bf16 (the weight gradients read bf16)
    const bool qpass = env_set("LNX_FP8_DGRAD_QPASS");  // A/B switch (read per call: the tests flip it): separate quantise passes over dY
    const bool mx_dgrad = c.dt == LNX_BF16 && fp8_rows(p, M, C) && k.fc2.off8ts != 0 && k.proj.off8ts != 0 && !p->dmask && C % 128 == 0 && !qpass;
    RUN(linear_dgrad(c, a, k.fc2, !(have_dy && p->dy8_ready), p->o_a8, p->o_a8s, p->o_h8, p->o_h8s));
    p->dy8_ready = false;
    if (p->dmask) RUN(lnx_dropout_mul(sA, c.dt, p->dmask + k.dm_hid, p->inv_keep, M, hid, c.st));  // through the dropout after the activation
    RUN(wfork(1));
    RUN(wgrad(cw, Mb, hid, C, sA, hid, c.at<void>(k.n2), C, k.fc1.param, k.fc1b, C, 0, 1, cm.m_dev));
    RUN(wdone(1));
    a = gemm_base(c, Mb, C, hid, sA, hid, c.wtptr(k.fc1), k.fc1.ld_t, sD, C, false);
    a.m_dev = cm.m_dev;
    RUN(linear_dgrad(c, a, k.fc1, false, p->o_h8, p->o_h8s));
    RUN(wjoin(0));  // norm2 backward overwrites sC
    // norm2 backward adds into g and, in the same pass, writes the attention branch's dY (DropPath-scaled g in storage type)
    Dx2 d2;
    d2.p = sC; d2.rowscale = p->drop_ptr(p->drop_attn[s][i]); d2.rps = rps; d2.inv = ca.inv; d2.nkeep = ca.nkeep;
    if (mx_dgrad) {
        d2.p8 = c.at<void>(p->o_a8); d2.p8s = c.at<void>(p->o_a8s);
    }
    // (CLS-only: the CLS rows of xmid / g by leading dimension, not by row map -- the second output's translation wants identity maps)
    RUN(ln_bwd(c, Mb, C, sD, c.dt, C, IDM, c.at<float>(k.xmid), LNX_F32, ldo, IDM, k.n2w, k.n2b, c.at<float>(k.mean2), c.at<float>(k.rstd2), g, g, LNX_F32, ldo, false, d2, cm));
    // ---- attention branch ----
    if (p->dmask) RUN(lnx_dropout_mul(sC, c.dt, p->dmask + k.dm_proj, p->inv_keep, M, C, c.st));  // through proj_drop
    RUN(wfork(2));
    RUN(wgrad(cw, Mb, C, C, sC, C, c.at<void>(k.o), ldo, k.proj.param, k.projb, C, 0, 2, pj_mdev));
    RUN(wdone(2));
    // CLS-only: the attention backward keeps its kernel and gets a dO that is zero outside the CLS rows (exact: a query with dO = 0 has
    // delta = 0 and dS = 0) -- one memset, and the B rows the product writes through its leading dimension
    if (lc) HIPRUN(hipMemsetAsync(sD, 0, (size_t)M * C * p->esz, (hipStream_t)c.st));
    a = gemm_base(c, Mb, C, C, sC, C, c.wtptr(k.proj), k.proj.ld_t, sD, ldo, false);
    a.m_dev = pj_mdev;
    RUN(linear_dgrad(c, a, k.proj, !mx_dgrad, p->o_a8, p->o_a8s));
    RUN(wjoin(1));  // the attention backward overwrites sA
    lnx_attn_bwd_args ab;
    memset(&ab, 0, sizeof ab);
    ab.dtype = c.dt; ab.B = B; ab.N = N; ab.E = E; ab.heads = heads; ab.head_dim = C / heads;
    ab.qkv = c.at<void>(k.qkvbuf); ab.cos_tab = c.at<float>(k.cos); ab.o = c.at<void>(k.o); ab.lse = c.at<float>(k.lse);
    ab.d_o = sD; ab.dqkv = sA; ab.freq_ws = c.at<float>(p->o_gcos); ab.delta = c.at<float>(p->o_delta);
    if (p->freq_defer && E < N) {  // the fold into dfreqs: one launch per backward segment (ln_flush)
        if (p->freq_pending == FREQ_DEFER_SLOTS) {
            RUN(lnx_attn_bwd_flush(c.st));
            p->freq_pending = 0;
        }
        ab.freq_ws = c.at<float>(p->o_gcos) + (int64_t)p->freq_pending * p->gcos_floats;
        ab.defer_freqs = 1;
        ++p->freq_pending;
    }
    ab.dsin_tab = c.at<float>(k.dsin); ab.dfreqs = p->G[k.freqs];
    if (p->c.rope_mode == LNX_ROPE_ROTATE) {
        ab.rope_mode = LNX_ROPE_ROTATE; ab.sin_tab = c.at<float>(k.dsin); ab.dsin_tab = nullptr; ab.grid_w = p->W[2 + s];
    }
    if (p->amask) {
        ab.drop_mask = p->amask + k.dm_attn; ab.drop_inv_keep = p->a_inv_keep;
    }
    {
        Timed t(c, 3, 14.0 * B * (double)N * N * C);
        RUN(lnx_attn_bwd_compact(&ab, ca.nkeep, p->gcos_floats, c.st));
    }
    RUN(wfork(3));
    RUN(wgrad(cw, M, 3 * C, C, sA, 3 * C, c.at<void>(k.n1), C, k.qkv.param, k.qkvb, C, 0, 3, ca.m_dev));
    RUN(lnx_gemm_tn_flush(cw.st));  // the four products' partial tiles -> their gradients, one launch
    RUN(wdone(3));
    RUN(wjoin(2));  // the qkv data gradient overwrites sC
    // (compact rows on either side of norm1's backward: its dy rows and the dx2 rows it writes are then different rows, so the in-place
    // hand-over below is off and this product writes sD, free since the attention backward read it)
    void* dn1 = (ca || cprev) ? sD : sC;
    a = gemm_base(c, M, C, 3 * C, sA, 3 * C, c.wtptr(k.qkv), k.qkv.ld_t, dn1, C, false);
    a.m_dev = ca.m_dev;
    RUN(gemm_nt_t(c, &a));
    // norm1 backward: g is final for this block; block i-1's MLP-branch dY goes into sC in place of this LN's dy (row-wise
    // in-place is safe: a row's dy is consumed before its statistics are known, its dx2 written after)
    Dx2 d1;
    if (prev_runs) {
        d1.p = sC; d1.rowscale = p->drop_ptr(p->drop_mlp[s][i - 1]); d1.rps = N; d1.inv = cprev.inv; d1.nkeep = cprev.nkeep;
        if (mx_dgrad) {  // block i - 1's fc2 data gradient reads it (same stage, same shapes: its own mx_dgrad is this one)
            d1.p8 = c.at<void>(p->o_a8); d1.p8s = c.at<void>(p->o_a8s);
            p->dy8_ready = true;
        }
    }
    RUN(ln_bwd(c, M, C, dn1, c.dt, C, IDM, c.at<float>(k.xin), LNX_F32, C, IDM, k.n1w, k.n1b, c.at<float>(k.mean1), c.at<float>(k.rstd1), g, g, LNX_F32, C, false, d1, ca));
    RUN(wjoin(3));  // the next kernel of the main stream may overwrite sA, and the block's gradients count as written from here on
    return 0;
}

// need_dx = false (the block is the cut: nothing before it trains): the depthwise data gradient, which only produces the block's input
// gradient, is not launched
int conv_block_bwd(const Ctx& c, int s, int i, float* g, bool need_dx) {
    lnx_plan* p = c.p;
    ConvBlk& k = p->conv[s][i];
    const int B = p->c.batch, H = p->H[s], W = p->W[s], C = p->c.dims[s];
    const int M = B * H * W;
    void* sA = c.at<void>(p->o_sA);
    void* sC = c.at<void>(p->o_sC);
    void* sD = c.at<void>(p->o_sD);
    Timed span(c, 9, 4.0 * M * C * (8.0 * C + 49.0));
    bool forked = false, joined = false;  // (only a block that forked work onto the weight-gradient stream waits for it)
    // the forward's list: sA / sB / sC then hold compact rows; sD keeps natural order, and the depthwise gradients skip the dropped samples
    const Compact cl = conv_compact_of(p, s, i);
    if (k.fused) {
        void* sB = c.at<void>(p->o_sB);
        lnx_convmlp_bwd_args f;
        memset(&f, 0, sizeof f);
        f.dtype = c.dt; f.M = M; f.C = C;
        f.g = g; f.ln = c.at<void>(k.ln); f.w1 = c.wptr(k.w1); f.b1 = p->P[k.b1];
        f.w2t = c.wtptr(k.w2); f.w1t = c.wtptr(k.w1); f.gamma = p->P[k.gamma];
        f.rowscale = p->drop_ptr(p->drop_conv[s][i]); f.rows_per_sample = H * W;
        f.act = sB; f.dh = sA; f.dz = sC; f.dln = sD; f.dgamma = p->G[k.gamma];
        f.dz_plain = 1;  // sC = rs g for the pwconv2 weight gradient, which then goes through lnx_layerscale_apply_wgrad
        f.perm = cl.perm; f.m_dev = cl.m_dev;
        if (k.fused_ln) {  // sD then holds the gradient wrt the depthwise conv output
            f.y = c.at<void>(k.y); f.ln_w = p->P[k.lnw]; f.mean = c.at<float>(k.mean); f.rstd = c.at<float>(k.rstd);
            f.d_ln_w = p->G[k.lnw]; f.d_ln_b = p->G[k.lnb];
            f.ws = c.at<float>(p->o_lnws); f.ws_floats = p->lnws_floats;
            if (p->ln_defer && p->o_lnws_defer != 0 && lnx_convmlp_bwd_ws_floats(C, M) <= p->lnws_defer_floats) {  // (as ln_bwd: folded at the segment's flush)
                RUN(ln_defer_slot(c, f.ws, f.ws_floats));
                f.ln_defer = 1;
            }
        }
        {
            Timed t(c, 7, 2.0 * M * C * 4 * C * 3);
            RUN(lnx_convmlp_bwd(&f, c.st));
        }
        const Ctx cw = wg_ctx(c);
        RUN(wg_fork(c, 0));  // the two pointwise weight gradients (and the LayerScale step behind them) beside the depthwise backward
        forked = true;
        // LayerScale gradient without z (include/lnx.h): the pwconv2 weight-gradient product runs on dY = rs g into zeroed scratch S | T,
        // then ONE launch adds gamma S / gamma T to the gradients and reads dgamma = rowdot(W2, S) + b2 T off them
        float* S = c.at<float>(p->o_lsws);
        float* T = S + (int64_t)C * 4 * C;
        HIPRUN(hipMemsetAsync(S, 0, ((size_t)C * 4 * C + C) * 4, (hipStream_t)cw.st));
        RUN(wgrad_into(cw, M, C, 4 * C, sC, C, sB, 4 * C, S, T, 4 * C, 0, cl.m_dev));
        RUN(wgrad(cw, M, 4 * C, C, sA, 4 * C, c.at<void>(k.ln), C, k.w1.param, k.b1, C, 0, 1, cl.m_dev));
        RUN(lnx_gemm_tn_flush(cw.st));
        RUN(lnx_layerscale_apply_wgrad(S, T, 4 * C, p->P[k.w2.param], p->P[k.b2], 4 * C, p->P[k.gamma], p->G[k.w2.param], p->G[k.b2], 4 * C, p->G[k.gamma], C, 4 * C, cw.st));
        RUN(wg_done(c, 0));
        if (!k.fused_ln) {  // the LayerNorm backward below overwrites sC
            RUN(wg_join(c, 0));
            joined = true;
        }
    } else {
        RUN(lnx_layerscale_bwd_ws(g, c.at<void>(k.z), c.dt, p->P[k.gamma], p->drop_ptr(p->drop_conv[s][i]), H * W, sC, p->G[k.gamma], M, C,
                                  p->det ? c.at<float>(p->o_detws) : nullptr, p->detws_floats, c.st));
        RUN(wgrad(c, M, C, 4 * C, sC, C, c.at<void>(k.act), 4 * C, k.w2.param, k.b2, 4 * C));
        lnx_gemm_args a = gemm_base(c, M, 4 * C, C, sC, C, c.wtptr(k.w2), k.w2.ld_t, sA, 4 * C, false);
        a.act = LNX_ACT_MUL_AUX; a.aux = c.at<void>(k.hpre); a.ldaux = 4 * C;  // what the forward left in hpre
        RUN(gemm_nt_t(c, &a));
        RUN(wgrad(c, M, 4 * C, C, sA, 4 * C, c.at<void>(k.ln), C, k.w1.param, k.b1, C));
        a = gemm_base(c, M, C, 4 * C, sA, 4 * C, c.wtptr(k.w1), k.w1.ld_t, sD, C, false);
        RUN(gemm_nt_t(c, &a));
    }
    void* dy = sD;  // gradient wrt the depthwise conv output
    if (!k.fused_ln) {
        RUN(ln_bwd(c, M, C, sD, c.dt, C, IDM, c.at<void>(k.y), c.dt, C, IDM, k.lnw, k.lnb, c.at<float>(k.mean), c.at<float>(k.rstd), nullptr, sC, c.dt, C, false));
        dy = sC;
    }
    lnx_dwconv_wgrad_args w;
    memset(&w, 0, sizeof w);
    w.B = B; w.H = H; w.W = W; w.C = C;
    w.x = c.at<float>(k.xin); w.x_dtype = LNX_F32; w.dy = dy; w.dy_dtype = c.dt;
    w.dw = p->G[k.dww]; w.db = p->G[k.dwb];
    if (p->det) {
        w.ws = c.at<float>(p->o_detws); w.ws_floats = p->detws_floats;
    }
    {
        Timed t(c, 5, (double)M * C * (4 + p->esz));
        RUN(lnx_dwconv7_wgrad_kept(&w, cl.perm, cl.nkeep, c.st));
    }
    lnx_dwconv_args d;
    memset(&d, 0, sizeof d);
    d.B = B; d.H = H; d.W = W; d.C = C;
    d.x = dy; d.x_dtype = c.dt; d.w49 = c.at<float>(k.w49); d.bias = nullptr; d.flip = 1; d.res = g; d.y = g; d.y_dtype = LNX_F32;
    if (need_dx) {
        Timed t(c, 4, (double)M * C * (8 + p->esz));  // bytes: read T dy + fp32 g, write fp32 g
        RUN(lnx_dwconv7_fwd_kept(&d, cl.perm, cl.nkeep, c.st));  // g of a dropped sample passes through unchanged
    }
    if (forked && !joined) RUN(wg_join(c, 0));  // the next block's kernels overwrite sA / sB / sC, and this block's gradients count as written from here on
    return 0;
}

// gradient of downsample i: gout (fp32, rows via gmap) -> gradient wrt the LN input
int downsample_bwd(const Ctx& c, int i, const float* gout, int64_t ldg, lnx_rowmap gmap, const void* x, int xdt, int64_t ldx, lnx_rowmap xm, void* dx, int dxdt,
                   int64_t lddx) {
    lnx_plan* p = c.p;
    Down& d = p->down[i];
    const int B = p->c.batch, Hin = p->H[i], Win = p->W[i], Cin = p->c.dims[i], Cout = p->c.dims[i + 1];
    const int Min = B * Hin * Win, Mout = Min / 4;
    void* sA = c.at<void>(p->o_sA);
    void* sC = c.at<void>(p->o_sC);
    RUN(lnx_scale_cast(gout, ldg, gmap, nullptr, 0, sC, c.dt, Cout, Mout, Cout, c.st));
    lnx_wgrad_args w;
    memset(&w, 0, sizeof w);
    w.dtype = c.dt; w.M = Mout; w.N = Cout; w.K = 4 * Cin;
    w.dY = sC; w.lddy = Cout; w.A = c.at<void>(d.ln); w.a_mode = LNX_ADDR_PATCH2; w.Hin = Hin; w.Win = Win; w.Cin = Cin;
    w.dW = p->G[d.w.param]; w.lddw = 4 * Cin; w.k_perm_c = Cin; w.db = p->G[d.cb];
    w.ws = c.at<float>(p->o_tnws); w.ws_floats = LNX_TN_WS_FLOATS;  // split-K partials through the workspace + reduce kernel, not by atomics (main stream only)
    {
        Timed t(c, 1, 2.0 * Mout * Cout * 4 * Cin);
        RUN(lnx_gemm_tn(&w, c.st));
    }
    lnx_gemm_args a = gemm_base(c, Mout, 4 * Cin, Cout, sC, Cout, c.wtptr(d.w), d.w.ld_t, sA, 0, false);
    a.c_mode = LNX_ADDR_PATCH2; a.Hin = Hin; a.Win = Win; a.Cin = Cin;
    RUN(gemm_nt_t(c, &a));
    RUN(ln_bwd(c, Min, Cin, sA, c.dt, Cin, IDM, x, xdt, ldx, xm, d.lnw, d.lnb, c.at<float>(d.mean), c.at<float>(d.rstd), nullptr, dx, dxdt, lddx, false));
    return 0;
}

int meta_head_bwd(const Ctx& cc, int s, int m, const float* g) {
    const Ctx c{cc.p, cc.st, LNX_F32};
    lnx_plan* p = c.p;
    MetaHead& k = p->meta[s][m];
    const int B = p->c.batch, C = p->c.dims[2 + s], N = p->Ntok[s];
    float* dtok = c.at<float>(p->o_mtmp[0]);   // [B, C] fp32
    void* t1 = c.at<void>(p->o_mtmp[1]);
    void* t2 = c.at<void>(p->o_mtmp[2]);
    float* dxf = c.at<float>(p->o_mtmp[3]);
    const lnx_rowmap rm = {1, N - 1, 1 + m};
    RUN(lnx_scale_cast(g, C, rm, nullptr, 0, dtok, LNX_F32, C, B, C, c.st));
    RUN(ln_bwd(c, B, C, dtok, LNX_F32, C, IDM, c.at<void>(k.h2), c.dt, C, IDM, k.nf2w, k.nf2b, c.at<float>(k.m2), c.at<float>(k.r2), nullptr, t1, c.dt, C, true));
    RUN(wgrad(c, B, C, C, t1, C, c.at<void>(k.n1), C, k.w2.param, k.b2, C));
    lnx_gemm_args a = gemm_base(c, B, C, C, t1, C, c.wtptr(k.w2), k.w2.ld_t, t2, C, false);
    RUN(gemm_nt_t(c, &a));
    RUN(ln_bwd(c, B, C, t2, c.dt, C, IDM, c.at<void>(k.h1), c.dt, C, IDM, k.nf1w, k.nf1b, c.at<float>(k.m1), c.at<float>(k.r1), nullptr, t1, c.dt, C, true));
    RUN(wgrad(c, B, C, C, t1, C, c.at<void>(k.x), C, k.w1.param, k.b1, C));
    a = gemm_base(c, B, C, C, t1, C, c.wtptr(k.w1), k.w1.ld_t, dxf, C, true);
    a.res = dtok; a.ldres = C;  // skip connection of ResNormLayer
    RUN(gemm_nt_t(c, &a));
    RUN(ln_bwd(c, B, C, dxf, LNX_F32, C, IDM, c.at<void>(k.h0), c.dt, C, IDM, k.lnw0, k.lnb0, c.at<float>(k.m0), c.at<float>(k.r0), nullptr, t1, c.dt, C, true));
    RUN(wgrad(c, B, C, 16, t1, C, c.at<void>(k.t0), 16, k.w0.param, k.b0, k.dim, k.dim));
    if (float* dmeta = p->dmeta_dst()) {  // t1 = this path's dp0 (fp32), overwritten by the next head: one launch per head
        const lnx_meta_input_grad_args ig = meta_input_grad_of(c, s, m, (const float*)t1);
        RUN(lnx_meta_input_grad(&ig, 1, dmeta, meta_width_of(p), meta_accumulates(s), c.st));
    }
    return 0;
}

// The metadata heads of stage s, backward: as meta_fwd
int meta_bwd(const Ctx& c, int s, const float* g) {
    if (c.p->chain_ok[s]) return meta_chain_bwd(c, s, g);
    for (int m = 0; m < c.p->c.n_meta; ++m) RUN(meta_head_bwd(c, s, m, g));
    return 0;
}

int tokens_bwd(const Ctx& c, int s, const float* g) {
    lnx_plan* p = c.p;
    const int B = p->c.batch, C = p->c.dims[2 + s], N = p->Ntok[s];
    const lnx_rowmap clsmap = {1, N - 1, 0};
    RUN(lnx_colsum_rows(g, C, clsmap, p->G[p->cls[s]], B, C, c.st));
    hipStream_t const mst = meta_stream(p);
    p->meta_forked[s] = mst != nullptr;
    if (mst) {
        // fork: the metadata-head backward only reads g; joined at the end of the segment (join_side)
        HIPRUN(hipEventRecord(p->ev_bfork[s], (hipStream_t)c.st));
        HIPRUN(hipStreamWaitEvent(mst, p->ev_bfork[s], 0));
        RUN(meta_bwd(Ctx{p, (void*)mst, c.dt}, s, g));
        HIPRUN(hipEventRecord(p->ev_bjoin[s], mst));
    } else {
        RUN(meta_bwd(c, s, g));
    }
    return 0;
}

// Recompute plans: bring block i's activations back into the stage's shared buffers (no-op when they are still there,
// i.e. for the last block of a stage right after the forward).  The block's output buffer is rewritten with the
// same values.
int conv_block_restore(const Ctx& c, int s, int i) {
    lnx_plan* p = c.p;
    if (!p->c.recompute || p->resident[s] == i) return 0;
    return conv_block_fwd(c, s, i, conv_out(p, s, i));
}
int rope_block_restore(const Ctx& c, int s, int i) {
    lnx_plan* p = c.p;
    if (!p->c.recompute || p->resident[2 + s] == i) return 0;
    p->dy8_ready = false;  // (the re-forward's LayerNorms write their MXFP8 activation copies into the same scratch)
    return rope_block_fwd(c, s, i, rope_out(p, s, i));
}

// the postponed LayerNorm column-sum reductions of this segment -> their gradients (one launch)
int ln_flush(const Ctx& c) {
    lnx_plan* p = c.p;
    if (p->ln_pending > 0) {
        RUN(lnx_layernorm_bwd_flush(c.st));
        p->ln_pending = 0;
    }
    if (p->freq_pending > 0) {  // ... and the attention backwards' freqs folds
        RUN(lnx_attn_bwd_flush(c.st));
        p->freq_pending = 0;
    }
    return 0;
}

int join_side(const Ctx& c, int s) {
    lnx_plan* p = c.p;
    if (p->meta_forked[s]) {  // (what tokens_bwd(s) did, whatever the mode has been switched to since)
        HIPRUN(hipStreamWaitEvent((hipStream_t)c.st, p->ev_bjoin[s], 0));
        p->meta_forked[s] = false;
    }
    return 0;
}

}  // namespace

extern "C" int lnx_plan_backward(lnx_plan* p, const float* dlogits, const float* dfeats, int segment, void* stream) {
    if (p && p->c.inference) FAIL("lnx_plan_backward: this plan was created for inference (cfg.inference = 1)");
    if (!p || !p->bound || !p->has_grads) FAIL("lnx_plan_backward: plan is not bound with gradient buffers");
    if (!p->fwd_done) FAIL("lnx_plan_backward: no forward to differentiate");
    if (lnx_get_deterministic() && !p->det)
        FAIL("lnx_plan_backward: deterministic mode is on but this plan was created with it off (its scratch and kernel choice do not fit the fixed-order routes): "
             "create the plan after lnx_set_deterministic(1)");
    if (segment < -1 || segment > 3) FAIL("lnx_plan_backward: bad segment %d", segment);
    // Postponed split-K second stages (lnx_wgrad_args.defer) are raw workspace / gradient pointers held per host thread: whatever an earlier
    // call that failed midway left behind is dropped here, and whatever THIS call leaves behind on an error path is dropped when it
    // returns (every block flushes its own products, so a call that succeeds leaves nothing).
    (void)lnx_gemm_tn_discard();
    (void)lnx_layernorm_bwd_discard();
    p->ln_pending = 0;
    (void)lnx_attn_bwd_discard();
    p->freq_pending = 0;
    struct TnGuard {
        lnx_plan* p;
        ~TnGuard() {
            (void)lnx_gemm_tn_discard();
            if (lnx_layernorm_bwd_discard() > 0) p->ln_pending = 0;  // (a successful call has flushed everything: nothing to drop)
            if (lnx_attn_bwd_discard() > 0) p->freq_pending = 0;
        }
    } tn_guard{p};
    const lnx_mformer_cfg& cf = p->c;
    if (segment <= 0) p->dy8_ready = false;
    Ctx c{p, stream, cf.dtype};
    hipStream_t st = (hipStream_t)stream;
    const int B = cf.batch;
    const int* D = cf.dims;
    const bool all = segment < 0;
    // Frozen prefix: a unit runs only if it is not before the cut (lnx_plan::runs); every unit that runs counts once per backward.  The
    // flushes and joins at the end of each segment stay: they act on whatever was postponed or forked, and on nothing otherwise.
    const int cut = p->cut;
    if (segment <= 0) p->bwd_units = 0;
    auto ran = [&]() { ++p->bwd_units; };

    if (all || segment == 0) {
        const int C = D[3];
        float* dfe = c.at<float>(p->o_tail[0]);  // d feats [B, C]
        bool have = false, heads_forked = false;
        const bool below_heads = cut < p->u_heads;  // (the heads as the cut: their weight and bias gradients only -- no features gradient)
        if (dfeats && below_heads) {
            HIPRUN(hipMemcpyAsync(dfe, dfeats, (size_t)B * C * 4, hipMemcpyDeviceToDevice, st));
            have = true;
        }
        if (cf.n_tasks > 0) {
            if (!dlogits) FAIL("lnx_plan_backward: dlogits is NULL");
            // one cast of the whole dlogits buffer (task blocks are contiguous, padding columns included); the heads' weight gradients go to the
            // weight-gradient stream (joined at the end of this segment), their data gradients are ONE accumulating launch
            unsigned char* dl0 = c.at<unsigned char>(p->o_dlT);
            RUN(lnx_scale_cast(dlogits, p->logits_numel, IDM, nullptr, 0, dl0, cf.dtype, p->logits_numel, 1, (int)p->logits_numel, stream));
            const Ctx cw = wg_ctx(c);
            RUN(wg_fork(c, 3));
            lnx_gemm_args hg[LNX_MAX_TASKS];
            for (int t = 0; t < cf.n_tasks; ++t) {
                const int ld = p->logit_ld[t], nc = cf.task_classes[t];
                void* dl = dl0 + p->logit_off[t] * p->esz;
                RUN(wgrad(cw, B, nc, C, dl, ld, c.at<void>(p->o_featsT), C, p->head_w[t].param, p->head_b[t], C));
                hg[t] = gemm_base(c, B, C, ld, dl, ld, c.wtptr(p->head_w[t]), p->head_w[t].ld_t, dfe, C, true);
            }
            RUN(wg_done(c, 3));
            heads_forked = true;
            if (have) {
                hg[0].res = dfe;
                hg[0].ldres = C;
            }
            if (below_heads) RUN(heads_nt(c, hg, cf.n_tasks, true));
            have = true;
        }
        if (!have && (below_heads || !dfeats)) FAIL("lnx_plan_backward: neither dlogits nor dfeats given");
        ran();  // heads
        float* dc1n = nullptr;
        float* g3 = c.at<float>(p->o_g[3]);
        if (p->runs(p->u_tail)) {
            // final_norm
            const float* fin_in = cf.only_last_cls ? c.at<float>(p->o_c2n) : c.at<float>(p->o_agg);
            float* dfin = c.at<float>(p->o_tail[1]);
            RUN(ln_bwd(c, B, C, dfe, LNX_F32, C, IDM, fin_in, LNX_F32, C, IDM, p->fin_w, p->fin_b, c.at<float>(p->o_fin_mean), c.at<float>(p->o_fin_rstd), nullptr,
                       dfin, LNX_F32, C, false));
            float* dc2n = dfin;
            if (!cf.only_last_cls) {
                dc1n = c.at<float>(p->o_tail[2]);
                dc2n = c.at<float>(p->o_tail[3]);
                RUN(lnx_agg2_bwd(dfin, c.at<float>(p->o_c1n), c.at<float>(p->o_c2n), p->P[p->agg_w], dc1n, dc2n, p->G[p->agg_w], p->G[p->agg_b], B, C, stream));
            }
            // norm_2 acts on the CLS row only: every other row of the stage-4 output has zero gradient
            if (cut < p->u_tail) HIPRUN(hipMemsetAsync(g3, 0, (size_t)B * p->Ntok[1] * C * 4, st));  // (tail as the cut: nobody reads g3)
            const lnx_rowmap clsrow = {1, p->Ntok[1] - 1, 0};
            RUN(ln_bwd(c, B, C, dc2n, LNX_F32, C, IDM, c.at<float>(p->o_stage_out[3]), LNX_F32, C, clsrow, p->norm_w[1], p->norm_b[1], c.at<float>(p->o_n2_mean),
                       c.at<float>(p->o_n2_rstd), nullptr, g3, LNX_F32, C, false));
            ran();
        }
        for (int i = cf.rope_depths[1] - 1; i >= 0 && p->runs(p->u_rope[1] + i); --i) {
            RUN(rope_block_restore(c, 1, i));
            RUN(rope_block_bwd(c, 1, i, g3, i != cf.rope_depths[1] - 1));
            ran();
        }
        if (p->runs(p->u_tok[1])) {
            RUN(tokens_bwd(c, 1, g3));
            ran();
        }
        if (p->runs(p->u_mid)) {
            // downsample 3 backward into d(norm_1 output); meta/CLS rows of dt1 start at zero
            const int C2 = D[2];
            void* dt1 = c.at<void>(p->o_dt1);
            HIPRUN(hipMemsetAsync(dt1, 0, (size_t)B * p->Ntok[0] * C2 * p->esz, st));
            const lnx_rowmap gm = {p->HW[3], p->E, p->E};
            const lnx_rowmap pm = {p->HW[2], p->E, p->E};
            RUN(downsample_bwd(c, 2, g3, C, gm, c.at<void>(p->o_t1), cf.dtype, C2, pm, dt1, cf.dtype, C2));
            if (!cf.only_last_cls) {
                void* du = c.at<void>(p->o_tail[4]);
                void* dca = c.at<void>(p->o_tail[5]);
                RUN(ln_bwd(c, B, C, dc1n, LNX_F32, C, IDM, c.at<float>(p->o_cl_u), LNX_F32, C, IDM, p->cl_lnw, p->cl_lnb, c.at<float>(p->o_cl_mean),
                           c.at<float>(p->o_cl_rstd), nullptr, du, cf.dtype, C, false));
                RUN(wgrad(c, B, C, C2, du, C, c.at<void>(p->o_cl_act), C2, p->cl_w2.param, p->cl_b2, C2));
                lnx_gemm_args a = gemm_base(c, B, C2, C, du, C, c.wtptr(p->cl_w2), p->cl_w2.ld_t, dca, C2, false);
                a.act = LNX_ACT_GELU_BWD; a.aux = c.at<void>(p->o_cl_hpre); a.ldaux = C2;
                RUN(gemm_nt_t(c, &a));
                RUN(wgrad(c, B, C2, C2, dca, C2, c.at<void>(p->o_t1), (int64_t)p->Ntok[0] * C2, p->cl_w1.param, p->cl_b1, C2));
                a = gemm_base(c, B, C2, C2, dca, C2, c.wtptr(p->cl_w1), p->cl_w1.ld_t, dt1, C2, false);
                a.c_map = lnx_rowmap{1, p->Ntok[0] - 1, 0};
                RUN(gemm_nt_t(c, &a));
            }
            float* g2 = c.at<float>(p->o_g[2]);
            // norm_1 backward also leaves the last stage-3 block's MLP-branch dY in sC (consumed first thing in segment 1) -- if that block runs
            Dx2 dn;
            if (p->runs(p->u_rope[0] + cf.rope_depths[0] - 1)) {
                dn.p = c.at<void>(p->o_sC); dn.rowscale = p->drop_ptr(p->drop_mlp[0][cf.rope_depths[0] - 1]); dn.rps = p->Ntok[0];
                const Compact cl = compact_of(p, p->drop_mlp[0][cf.rope_depths[0] - 1], B * p->Ntok[0], C2, p->Ntok[0]);
                dn.inv = cl.inv; dn.nkeep = cl.nkeep;
            }
            RUN(ln_bwd(c, B * p->Ntok[0], C2, dt1, cf.dtype, C2, IDM, c.at<float>(p->o_stage_out[2]), LNX_F32, C2, IDM, p->norm_w[0], p->norm_b[0],
                       c.at<float>(p->o_t1_mean), c.at<float>(p->o_t1_rstd), nullptr, g2, LNX_F32, C2, false, dn));
            ran();
        }
        // the stage-4 metadata-head backward (side stream, ~10 small fp32 GEMMs) is joined at the END OF SEGMENT 1: it only
        // produces parameter gradients, and joining here exposed most of its ~0.7 ms behind the three downsample kernels.
        // That holds for segment-wise callers too (segments run 0..3 in order): the gradients of the stage-4 metadata heads
        // are reported as final after segment 1, those of the stage-3 heads after segment 2 (lnx_plan_segment_params).
        RUN(ln_flush(c));
        if (heads_forked) RUN(wg_join(c, 3));  // (the weight-gradient stream runs in order: every RoPE block's joins already imply this one)
    }
    if (all || segment == 1) {
        float* g2 = c.at<float>(p->o_g[2]);
        for (int i = cf.rope_depths[0] - 1; i >= 0 && p->runs(p->u_rope[0] + i); --i) {
            RUN(rope_block_restore(c, 0, i));
            RUN(rope_block_bwd(c, 0, i, g2, true));
            ran();
        }
        if (p->runs(p->u_tok[0])) {
            RUN(tokens_bwd(c, 0, g2));
            ran();
        }
        if (p->runs(p->u_down[1])) {
            const lnx_rowmap gm = {p->HW[2], p->E, p->E};
            RUN(downsample_bwd(c, 1, g2, D[2], gm, c.at<float>(p->o_stage_out[1]), LNX_F32, D[1], IDM, c.at<float>(p->o_g[1]), LNX_F32, D[1]));
            ran();
        }
        RUN(ln_flush(c));
        RUN(join_side(c, 1));
    }
    if (all || segment == 2) {
        float* g1 = c.at<float>(p->o_g[1]);
        for (int i = cf.conv_depths[1] - 1; i >= 0 && p->runs(p->u_conv[1] + i); --i) {
            RUN(conv_block_restore(c, 1, i));
            RUN(conv_block_bwd(c, 1, i, g1, cut < p->u_conv[1] + i));
            ran();
        }
        if (p->runs(p->u_down[0])) {
            RUN(downsample_bwd(c, 0, g1, D[1], IDM, c.at<float>(p->o_stage_out[0]), LNX_F32, D[0], IDM, c.at<float>(p->o_g[0]), LNX_F32, D[0]));
            ran();
        }
        RUN(ln_flush(c));
        RUN(join_side(c, 0));  // stage-3 metadata heads: hidden behind the whole ConvNeXt stage-2 backward
    }
    if (all || segment == 3) {
        float* g0 = c.at<float>(p->o_g[0]);
        for (int i = cf.conv_depths[0] - 1; i >= 0 && p->runs(p->u_conv[0] + i); --i) {
            RUN(conv_block_restore(c, 0, i));
            RUN(conv_block_bwd(c, 0, i, g0, cut < p->u_conv[0] + i));
            ran();
        }
        if (p->runs(0)) {  // the stem
            const int M0 = B * p->HW[0];
            void* sC = c.at<void>(p->o_sC);
            RUN(ln_bwd(c, M0, D[0], g0, LNX_F32, D[0], IDM, c.at<void>(p->o_stem_pre), cf.dtype, D[0], IDM, p->stem_lnw, p->stem_lnb, c.at<float>(p->o_stem_mean),
                       c.at<float>(p->o_stem_rstd), nullptr, sC, cf.dtype, D[0], false));
            const int kst = cf.in_chans * 16;
            RUN(wgrad(c, M0, D[0], 64, sC, D[0], c.at<void>(p->o_patches), 64, p->stem_w.param, p->stem_b, kst, kst));
            if (p->want_x && p->dx_out && !p->hold_input_grads) {
                // the image gradient: dx = unpatchify(dY . W) from the same dY, in one kernel where it carries the geometry
                if (p->stem_w.ld_t == 0) {
                    lnx_stem_dgrad_args a;
                    memset(&a, 0, sizeof a);
                    a.dtype = cf.dtype; a.B = B; a.Cin = cf.in_chans; a.H = cf.img_h; a.W = cf.img_w; a.Cout = D[0];
                    a.dy = sC; a.ldy = D[0]; a.w = c.wptr(p->stem_w); a.dx = p->dx_out;
                    RUN(lnx_stem_dgrad(&a, stream));
                } else {
                    void* dcol = c.at<void>(p->o_dcol);
                    // (the product leaves the GEMM in fp32: dx is an fp32 tensor, and a bf16 round trip in between would be its only rounding)
                    const lnx_gemm_args a = gemm_base(c, M0, kst, D[0], sC, D[0], c.wtptr(p->stem_w), p->stem_w.ld_t, dcol, kst, true);
                    RUN(gemm_nt_t(c, &a));
                    RUN(lnx_col2im_stem(dcol, LNX_F32, kst, B, cf.in_chans, cf.img_h, cf.img_w, p->dx_out, stream));
                }
            }
            ran();
        }
        RUN(ln_flush(c));
    }
    return 0;
}

// The gradient pointers are read only while launches are built: every postponed LayerNorm / split-K / freqs reduction holding
// one is flushed before lnx_plan_backward returns, and the weight-gradient stream's kernels captured theirs at enqueue time.
// So swapping the pointer set for the call is all it takes; no rebind (which would sync and clear the forward).
extern "C" int lnx_plan_backward_into(lnx_plan* p, const float* dlogits, const float* dfeats, float* const* grads, void* stream) {
    if (!p || !grads) FAIL("lnx_plan_backward_into: null %s", !p ? "plan" : "gradient pointer set");
    if (!p->bound || !p->has_grads) FAIL("lnx_plan_backward_into: plan is not bound with gradient buffers");
    const size_t n = p->names.size();
    for (size_t i = 0; i < n; ++i)
        if (grads[i] == nullptr || (((uintptr_t)grads[i]) & 3) != 0) FAIL("lnx_plan_backward_into: gradient of %s is null or misaligned", p->names[i].c_str());
    std::vector<float*> into(grads, grads + n);
    struct Swap {
        lnx_plan* p;
        std::vector<float*>& v;
        Swap(lnx_plan* p_, std::vector<float*>& v_) : p(p_), v(v_) {
            p->G.swap(v);
            p->hold_input_grads = true;  // a per-task backward never writes the input gradients (include/lnx.h)
        }
        ~Swap() {  // the bound set is back on every exit path
            p->G.swap(v);
            p->hold_input_grads = false;
        }
    } swap{p, into};
    return lnx_plan_backward(p, dlogits, dfeats, -1, stream);
}

extern "C" int lnx_plan_segment_params(const lnx_plan* p, int segment, int* idx_out, int max_out) {
    if (!p || segment < 0 || segment > 3) return -1;
    int n = 0;
    for (size_t i = 0; i < p->seg.size(); ++i)
        if (p->seg[i] == segment) {
            if (idx_out && n < max_out) idx_out[n] = (int)i;
            ++n;
        }
    return n;
}

static int profile_begin(lnx_plan* p, bool spans, const char* who) {
    if (!p) FAIL("%s: null plan", who);
    p->profile = true;
    p->profile_spans = spans;
    p->spans.clear();
    p->ev_used = 0;
    return 0;
}
extern "C" int lnx_plan_profile_begin(lnx_plan* p) { return profile_begin(p, false, "lnx_plan_profile_begin"); }
extern "C" int lnx_plan_profile_begin_spans(lnx_plan* p) { return profile_begin(p, true, "lnx_plan_profile_begin_spans"); }

extern "C" int lnx_plan_set_wgrad_stream(lnx_plan* p, int on) {
    if (!p || (on != 0 && on != 1)) {
        lnx_set_error("lnx_plan_set_wgrad_stream: %s", !p ? "null plan" : "on must be 0 or 1");
        return -1;
    }
    const int was = wg_on(p) ? 1 : 0;
    if (p->wgs) (void)hipStreamSynchronize(p->wgs);  // (every block joins before it returns: nothing is pending unless a call failed half-way)
    p->wgs_on = on != 0;
    return was;
}

extern "C" int lnx_plan_set_meta_stream(lnx_plan* p, int mode) {
    if (!p || mode < 0 || mode > 2) {
        lnx_set_error("lnx_plan_set_meta_stream: null plan / mode %d (0 launch stream, 1 side stream, 2 weight-gradient stream)", mode);
        return -1;
    }
    const int was = p->meta_mode;
    if (mode == 1 && p->side == nullptr) mode = 0;  // LNX_NO_SIDE_STREAM: the side stream was never created
    p->meta_mode = mode;
    return was;
}

// Ends profiling; synchronises the device and returns, per kernel class, the summed launch
// time (ms), the summed algorithmic work (FLOPs, or bytes for the HBM-bound classes) and the
// number of launches.  Arrays must hold LNX_PROFILE_CLASSES entries.
static int profile_collect(lnx_plan* p, int ncls, double* ms, double* work, double* bytes, int* launches) {
    p->profile = false;
    p->profile_spans = false;
    HIPRUN(hipDeviceSynchronize());
    for (int i = 0; i < ncls; ++i) {
        ms[i] = 0;
        work[i] = 0;
        if (bytes) bytes[i] = 0;
        launches[i] = 0;
    }
    for (const auto& sp : p->spans) {
        if (sp.cls >= ncls) continue;
        float t = 0.f;
        HIPRUN(hipEventElapsedTime(&t, sp.e0, sp.e1));
        ms[sp.cls] += t;
        work[sp.cls] += sp.work;
        if (bytes) bytes[sp.cls] += sp.bytes;
        launches[sp.cls] += 1;
    }
    p->spans.clear();
    p->ev_used = 0;
    return 0;
}

extern "C" int lnx_plan_profile_end(lnx_plan* p, double* ms, double* work, int* launches) {
    if (!p || !ms || !work || !launches) FAIL("lnx_plan_profile_end: null argument");
    return profile_collect(p, LNX_PROFILE_CLASSES, ms, work, nullptr, launches);
}

extern "C" int lnx_plan_profile_end_ex(lnx_plan* p, double* ms, double* work, double* bytes, int* launches) {
    if (!p || !ms || !work || !bytes || !launches) FAIL("lnx_plan_profile_end_ex: null argument");
    return profile_collect(p, LNX_PROFILE_CLASSES_EX, ms, work, bytes, launches);
}
