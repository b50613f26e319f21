/*
 * lnx.h -- C ABI of the MI355X-native mFormerV1 forward/backward path.
 *
 * This is the drop-in boundary: plain C symbols taking raw device
 * pointers, sizes and a hipStream_t (passed as void*).  No torch types, no allocation
 * inside (workspaces are passed in), no hidden synchronisation: every call only enqueues
 * work on the given stream.  Every function returns 0 on success; on failure a message
 * is available from lnx_last_error().
 *
 * Each entry replaces work the reference does through torch.nn leaf modules; the
 * reference file:line it stands for is cited next to it (paths under /root/reference/).
 *
 * dtype codes: LNX_F32 = 0 (strict-parity mode), LNX_BF16 = 1 (production).  `dtype`
 * always names the storage type T of activations / GEMM operands; accumulation,
 * statistics, the residual stream, parameters and gradients are fp32.
 */
#ifndef LNX_H
#define LNX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LNX_F32 0
#define LNX_BF16 1

const char* lnx_last_error(void);
int lnx_version(void);
/* number of compute units of the current device (used to size grids) */
int lnx_device_cus(void);
/* Persistent kernels (gemm_nt_v7 / v9, the resident-weight conv-MLP kernels, the depthwise kernels: one workgroup per CU that
 * draws tiles from atomic counters) launch on (compute units - margin) CUs.  Default 0, or LNX_CU_MARGIN from the environment at
 * first use.  With the counters a workgroup that cannot be placed beside a resident collective kernel costs nothing (the others
 * take its tiles); a margin only spares the hardware the queue of unplaceable workgroups.  Replaces nothing in the reference:
 * torch DDP's NCCL kernels and cuBLAS share the SMs the same way (linnaeus/main.py:936-983). */
int lnx_set_cu_margin(int cus);
/* Deterministic mode: with it on, every reduction of the training path (forward, backward, losses, optimizers) takes a fixed-order
 * route -- one contributor per output element, or per-contributor partial sums in caller-provided scratch that a second stage folds
 * in index order and adds to the destination once -- and the persistent kernels stride over their tiles instead of drawing them.  The
 * same inputs then give the same bits, run to run, on one GPU, one library build, one batch shape, one CU margin and one set of
 * LNX_* switches (those change grids and split counts, hence the order).  Off by default: nothing changes then.  The value is
 * process-wide and read per launch; its initial value is LNX_DETERMINISTIC=1 from the environment, read once.  An entry point that
 * has no fixed-order route for what it is asked (missing scratch, a kernel that sums with float atomics only) refuses by name
 * through lnx_last_error instead of taking the other route.  lnx_set_deterministic returns the previous value. */
int lnx_set_deterministic(int on);
int lnx_get_deterministic(void);
/* 1 while the persistent kernels stride over their tiles (LNX_TILE_SCHED=static, or the deterministic mode), 0 while they draw them */
int lnx_tile_sched_static(void);

/* Row map for token buffers that carry E extra rows per sample:
 * phys_row = m + (m / group) * pad + off   (group == 0: identity). */
typedef struct lnx_rowmap {
    int group, pad, off;
} lnx_rowmap;

/* ------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue(A[M,K] . W[N,K]^T)         (MFMA, fp32 accumulate)
 * Replaces nn.Linear / nn.Conv2d(k=s) forward and their data-gradients:
 *   pwconv1/pwconv2 blocks/convnext.py:60-64,79-81; qkv/proj rope_2d_mhsa.py:292-294;
 *   fc1/fc2 blocks/mlp.py:36-39; stem/downsample convs mFormerV1.py:146, convnext.py:110;
 *   heads heads/linear_head.py:27; meta heads mFormerV1.py:291-306.
 * -----------------------------------------------------------------------------------*/
enum { LNX_ACT_NONE = 0, LNX_ACT_GELU = 1, LNX_ACT_RELU = 2, LNX_ACT_GELU_BWD = 3, LNX_ACT_RELU_BWD = 4,
       /* round 3: the derivative is evaluated ONCE, in the forward, where the pre-activation is at hand in fp32 (the polynomial erf
        * and the exponential are the dominant VALU cost of both epilogues; the backward GEMM's becomes one multiply):
        * GELU_D   forward:  C = GELU(v) and c2 = GELU'(v) (instead of v)           -- c2 is required
        * MUL_AUX  backward: v *= aux                                               -- aux = that c2 */
       LNX_ACT_GELU_D = 5, LNX_ACT_MUL_AUX = 6 };
enum { LNX_ADDR_PLAIN = 0, LNX_ADDR_PATCH2 = 1 };

typedef struct lnx_gemm_args {
    int dtype;           /* T of A, W, aux, c2 (and of C unless out_f32) */
    int M, N, K;         /* K must be a multiple of 16/sizeof(T) */
    const void* A;       /* [M, K] rows, leading dimension lda (elements) */
    int64_t lda;
    const void* W;       /* [N, K] rows (torch Linear layout), leading dimension ldw */
    int64_t ldw;
    void* C;             /* [M, N] */
    int64_t ldc;
    int out_f32;         /* 1: C is fp32, 0: C is T */
    /* A addressing: PLAIN, or PATCH2 = gather 2x2/stride-2 patches from an NHWC tensor
     * [B, Hin, Win, Cin] with k = (kh*2 + kw)*Cin + c  (then K == 4*Cin, M == B*Hin/2*Win/2) */
    int a_mode, Hin, Win, Cin;
    /* C addressing: PLAIN with row map, or PATCH2 = scatter into NHWC (data-gradient of
     * the 2x2 conv; then N == 4*Cin and Hin/Win/Cin describe the destination) */
    int c_mode;
    lnx_rowmap c_map;
    /* epilogue, in this order: v = acc + bias[n]; c2 = v; act; v *= gamma[n];
     * v *= rowscale[m / rows_per_sample]; v += res[row, n]; C = v */
    const float* bias;     /* [N] or NULL */
    void* c2;              /* optional second output [M, N] of T, leading dimension ldc2 */
    int64_t ldc2;
    int act;
    const void* aux;       /* GELU_BWD: pre-activation, RELU_BWD: activation output; T */
    int64_t ldaux;
    const float* gamma;    /* [N] or NULL (LayerScale, blocks/convnext.py:82-83) */
    const float* rowscale; /* per-sample DropPath multiplier or NULL (drop_path.py:29-33) */
    int rows_per_sample;
    const float* res;      /* fp32 residual with the addressing of C, or NULL */
    int64_t ldres;
    void* c8;              /* lnx_gemm_nt_mxfp8 only, optional: MXFP8 copy of the bf16 output C (exactly lnx_quantize_mxfp8 of C), */
    int64_t ldc8;          /* ldc8 bytes per row, block scales in c8_scales ([N/128][M][4]); needs N % 128 == 0 and the */
    void* c8_scales;       /* bias + GELU + pre-activation form or the GELU' form (the fc1 -> fc2 hand-over of the model's fp8 mode
                              and its mirror image in the backward) */
    /* Compact rows (DropPath compaction lists, below), lnx_gemm_nt only (the fp8 entry points refuse them):
     * m_dev  optional device int: the product covers the rows m < min(M, *m_dev), read once at kernel entry.  The launch is sized
     *        from M on the host; rows >= the effective count of A / aux are never read into a result and rows >= it of C / c2 are
     *        never written (they may hold anything, NaN included; all M rows must be allocated).  NULL: all M rows.
     * perm   optional sample permutation [M / rows_per_sample] (device ints) for the residual forms: compact row m stands for sample
     *        b = perm[m / rows_per_sample], so rowscale is read at b and res / C are addressed at row b * rows_per_sample + m %
     *        rows_per_sample; A, aux and c2 stay compact (row m).  Needs res and rowscale (refused without), plain C addressing and an
     *        identity c_map.  Rows of C that
     *        belong to samples behind the effective count are not touched.  NULL: identity. */
    const int* m_dev;
    const int* perm;
} lnx_gemm_args;

int lnx_gemm_nt(const lnx_gemm_args* args, void* stream);

/* Several small products in ONE launch (a wave per 32 x 32 output tile, operands straight from L2): what the model's tail needs for its
 * classification heads (mFormerV1.py:536-541) -- the same M = batch product once per head, forward and data gradient.
 *   accumulate == 0: n independent problems, each with its own A / W / C / bias / res / M / N / K (e.g. logits_t = feats . W_t^T + b_t);
 *   accumulate == 1: C = bias + res + sum_j A_j . W_j^T in one accumulator chain (e.g. d feats = sum_t dlogits_t . W_t); M, N, C, ldc,
 *                    bias, res are taken from problem 0, A / lda / W / ldw / K from every problem.
 * bf16 operands, plain addressing, no activation / scales / second output; all problems the same out_f32.  lnx_gemm_nt_group_ok says
 * (host side, no device work) whether a list qualifies; lnx_gemm_nt_group fails loudly on one that does not. */
#define LNX_GEMM_GROUP_MAX 8
int lnx_gemm_nt_group_ok(const lnx_gemm_args* problems, int n, int accumulate);
int lnx_gemm_nt_group(const lnx_gemm_args* problems, int n, int accumulate, void* stream);

/* Which kernel family the NT dispatchers (lnx_gemm_nt, lnx_gemm_nt_fp8, lnx_gemm_nt_mxfp8) chose (host-side bookkeeping, no device work): the parity tests use it to prove
 * that a shape really ran on the kernel it is meant to cover (e.g. the persistent gemm_nt_v7 at the benchmark's M = 50 944).
 * lnx_last_nt_kernel(): family of the most recent NT launch of this process (any stream), 0 before the first.
 * lnx_nt_kernel_launches(kind): launches of that family since the library was loaded. */
enum { LNX_NT_KERNEL_NONE = 0, LNX_NT_KERNEL_V1 = 1 /* 128x128 register-staged, both storage types */, LNX_NT_KERNEL_V2 = 2 /* 256x128 LDS-DMA ring */,
       LNX_NT_KERNEL_SKINNY = 3 /* M <= 256, one wave per tile */, LNX_NT_KERNEL_V4 = 4 /* 256x256 tile */,
       LNX_NT_KERNEL_FP8 = 6 /* lnx_gemm_nt_fp8 / _mxfp8 on the 128x128 tile */, LNX_NT_KERNEL_V7 = 7 /* persistent 256x128, deferred stores */,
       LNX_NT_KERNEL_MX8 = 8 /* lnx_gemm_nt_mxfp8 on the 256x256 tile (gemm_nt_mx8_kernel) */, LNX_NT_KERNEL_V9 = 9 /* persistent 256x256 (round 4) */,
       LNX_NT_KERNEL_EXPERIMENT = 15 /* a kernel of tools/experiments/ (never in the shipped library) */, LNX_NT_KERNEL_KINDS = 16 };
int lnx_last_nt_kernel(void);
int64_t lnx_nt_kernel_launches(int kind);
/* The family lnx_gemm_nt WOULD launch for these arguments (no launch, no device work, no GPU needed; negative on bad arguments): only
 * M / N / K / dtype / out_f32 / act / a_mode / c_mode and WHICH optional operands are non-NULL are looked at, never the memory behind
 * them.  DESIGN.md's dispatch table is checked against this by tests/test_host_logic.py. */
int lnx_nt_dispatch(const lnx_gemm_args* args);

/* fp8 operands (BASELINE config 5's "fp8 MFMA path"; the reference has no fp8 code: this is the MI355X form of its
 * bf16 Linear, mlp.py:46-66 / rope_2d_mhsa.py:432,500).  OCP e4m3fn storage, one dequantisation scale per tensor:
 *   lnx_amax          amax[0] = max(amax[0], max |x|)            (device scalar, caller zeroes it)
 *   lnx_quantize_fp8  y = e4m3(x * 448 / amax[0]),  scale_out[0] = amax[0] / 448   (amax 0 -> scale 1)
 *   lnx_gemm_nt_fp8   C = epilogue( a_scale[0] * w_scale[0] * A8 . W8^T ): `args` as lnx_gemm_nt with dtype = LNX_BF16
 *                     for C / c2 / aux, but A and W are e4m3 bytes (lda / ldw in bytes), K % 128 == 0, N % 16 == 0, M >= 256, plain
 *                     addressing and an epilogue the specialised forms cover (bias, GELU + c2, GELU', fp32 residual).
 * The product runs on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales: 2x the bf16 MFMA rate. */
int lnx_amax(const void* x, int x_dtype, int64_t ldx, int rows, int cols, float* amax, void* stream);
int lnx_quantize_fp8(const void* x, int x_dtype, int64_t ldx, int rows, int cols, const float* amax, void* y, int64_t ldy, float* scale_out, void* stream);
int lnx_gemm_nt_fp8(const lnx_gemm_args* args, const float* a_scale, const float* w_scale, void* stream);

/* MXFP8 (OCP microscaling): e4m3 elements, one E8M0 (power-of-two) scale per 32 consecutive elements of a row; the block
 * scales are operands of v_mfma_scale_f32_16x16x128_f8f6f4 itself, so there is no amax pass, no scale state and no
 * dequantisation step -- the CDNA4-native form of the fp8 path.
 *   lnx_quantize_mxfp8  per block: e = smallest exponent with amax * 2^-e <= 448, y = e4m3(x * 2^-e) (round to nearest even),
 *                       scales: bytes [cols/128][rows][4], byte j of (ks, r) = e + 127 of block 4 ks + j of row r
 *                       (cols % 128 == 0; x fp32 or bf16, 16-byte aligned rows; ldy in bytes)
 *   lnx_gemm_nt_mxfp8   C = epilogue( dequant(A8) . dequant(W8)^T ): `args` as lnx_gemm_nt_fp8, a_scales [K/128][M][4],
 *                       w_scales [K/128][N][4] as written by lnx_quantize_mxfp8 */
int lnx_quantize_mxfp8(const void* x, int x_dtype, int64_t ldx, int rows, int cols, void* y, int64_t ldy, void* scales, void* stream);
int lnx_gemm_nt_mxfp8(const lnx_gemm_args* args, const void* a_scales, const void* w_scales, void* stream);

/* Weight gradient  dW[N,K] += dY[M,N]^T . A[M,K]  and optionally db[N] += colsum(dY).
 * Split over M across workgroups.  Partial tiles are added to dW/db with fp32 atomics, or, when the
 * caller passes a workspace (ws), stored there and summed into dW/db by a second kernel in a fixed
 * order (faster: no memory-side atomics; and bit-reproducible).  dW/db accumulate: caller zeroes them.
 * Default mode: sparsely filled tiles, a missing or too small workspace and the fp32 / odd-M kernel take the atomics.
 * Deterministic mode (lnx_set_deterministic): two or more splits always meet in the workspace second stage; where it is missing or too
 * small (and in the kernel that has no second stage) the contraction is split less, down to one workgroup per output tile -- one
 * contributor per element.
 * Replaces autograd's weight/bias gradient of every Linear/patchify conv above. */
typedef struct lnx_wgrad_args {
    int dtype;
    int M, N, K;
    const void* dY; /* [M, N] of T */
    int64_t lddy;
    const void* A;  /* [M, K] of T (PLAIN) or NHWC source (PATCH2) */
    int64_t lda;
    int a_mode, Hin, Win, Cin;
    float* dW;      /* [N, ldw] fp32 */
    int64_t lddw;
    int k_perm_c;   /* >0: K = P*k_perm_c with k = p*C + c stored at column c*P + p
                       (torch conv weight layout [N, C, kh, kw]) */
    float* db;      /* [N] or NULL */
    int splits;     /* 0: choose automatically */
    int k_store;    /* >0: only columns k < k_store are stored (zero-padded K) */
    float* ws;      /* optional split-K workspace (device), NULL = atomics (deterministic mode: NULL = fewer splits, down to one) */
    int64_t ws_floats; /* its size; LNX_TN_WS_FLOATS always suffices */
    int defer;      /* round 4.  != 0 (and ws given): the product leaves its split-K partial tiles in ws and the summation into dW / db
                       is postponed to lnx_gemm_tn_flush(), which sums the partial tiles of ALL postponed products of this host thread
                       in one launch (up to 8; a ninth, or one on another stream, flushes first).  Every pending product needs its
                       own ws, untouched until the flush; dW / db are final only after it. */
    const int* m_dev; /* optional device int (DropPath compaction lists, below: a list's m_eff): the contraction runs over the rows
                       m < min(M, *m_dev) only.  The launch (splits, workspace) is sized from M on the host; every split takes its
                       contraction range from the effective count inside the kernel, a split left without rows adds nothing (its
                       workspace tiles are zeros).  Rows >= the effective count of dY and A are never multiplied in: they may hold
                       anything, NaN included -- they must exist, though (M rows are allocated).  NULL: all M rows. */
} lnx_wgrad_args;
#define LNX_TN_WS_FLOATS (256 * (256 * 128 + 256))

int lnx_gemm_tn(const lnx_wgrad_args* args, void* stream);
/* What lnx_gemm_tn WOULD launch for these arguments (no launch, no device work, no GPU needed; 0 on success, 1 and lnx_last_error on
 * arguments lnx_gemm_tn refuses for their sizes): only dtype / M / N / K / leading dimensions / a_mode and its geometry / k_store /
 * splits / ws_floats, WHICH of ws is non-NULL, the deterministic mode and the LNX_GEMM_V1 / LNX_TN_ORIENT / LNX_TN_ATOMIC switches are
 * looked at, never the memory behind a pointer.  It is the function lnx_gemm_tn itself takes its launch from; the seam tests use it to
 * prove which kernel, tile form, split and summation path a case ran on, and DESIGN.md's TN table is checked against it. */
enum { LNX_TN_KERNEL_V1 = 1 /* gemm_tn_kernel<T>: 128x128 register-staged, fp32 and bf16, atomics only */,
       LNX_TN_KERNEL_RING = 2 /* gemm_tn_v2_kernel<rw, cw, patch>: LDS-DMA ring of 64-row contraction tiles, bf16 */ };
typedef struct lnx_tn_launch {
    int kernel;          /* LNX_TN_KERNEL_* */
    int rw, cw;          /* output tile: rows (of N) x columns (of K); 128 x 128, 256 x 128 or 128 x 256 */
    int patch;           /* 1: the 2x2 patch-gather instantiation (ring kernel) / addressing (128x128 kernel) */
    int tiles_n, tiles_k;
    int splits;          /* workgroups per output tile as launched ... */
    int m_per_split;     /* ... and the contraction rows each of them covers (the last one what is left) */
    int workspace;       /* 1: partial tiles go through ws and the second stage; 0: fp32 atomics on dW / db */
} lnx_tn_launch;
int lnx_gemm_tn_query(const lnx_wgrad_args* args, lnx_tn_launch* out);
/* sums the partial tiles of the products postponed with `defer` into their dW / db (no-op when nothing is pending).  `stream` must be the
 * stream those products were launched on (or NULL = that stream): another stream is an error (the reduces would be ordered behind the wrong work). */
int lnx_gemm_tn_flush(void* stream);
/* forgets this host thread's postponed products WITHOUT summing them (returns how many): for a caller whose step failed between a
 * postponed product and its flush -- the descriptors hold raw ws / dW / db pointers that must not outlive those buffers.
 * lnx_plan_backward does this itself on entry and on every error path, lnx_plan_destroy on teardown. */
int lnx_gemm_tn_discard(void);


/* ------------------------------------------------------------------------------------
 * LayerNorm over the last dimension C (biased variance, eps inside the sqrt).
 * In NHWC memory this is also the reference's LayerNormChannelsFirst.
 *   nn.LayerNorm: blocks/convnext.py:59, rope_2d_mhsa.py:546-547, mFormerV1.py:271-273,
 *   294,320-328, res_norm_layer.py:18-19; LayerNormChannelsFirst: blocks/convnext.py:21-43.
 * -----------------------------------------------------------------------------------*/
typedef struct lnx_ln_args {
    int M, C;
    float eps;
    const void* x;      /* rows via x_map, leading dimension ldx */
    int x_dtype;
    int64_t ldx;
    lnx_rowmap x_map;
    const float* w;     /* [C] */
    const float* b;     /* [C] */
    void* y;            /* rows via y_map */
    int y_dtype;
    int64_t ldy;
    lnx_rowmap y_map;
    const void* add;    /* optional [M, C] of x_dtype added to the output (ResNormLayer skip) */
    int64_t ldadd;      /* a multiple of 4, as ldx / ldy */
    float* mean;        /* [M] or NULL */
    float* rstd;        /* [M] or NULL */
    void* y8;           /* optional second output: MXFP8 copy of the bf16 output (exactly lnx_quantize_mxfp8 of y), compact rows
                           (row m), ldy8 bytes per row, block scales in y8_scales ([C/128][M][4]).  Needs x fp32, y bf16,
                           an identity y_map and C % 128 == 0: the producer side of the model's fp8 mode. */
    int64_t ldy8;
    void* y8_scales;
    /* Compact rows (DropPath compaction lists, below): a sample gather on the x side.
     * perm    optional [M / rows_per_sample]: output row m (y, mean, rstd: compact) is the LayerNorm of x row
     *         perm[m / rows_per_sample] * rows_per_sample + m % rows_per_sample.  Needs an identity x_map, no add, no y8.
     * m_dev   optional device int: rows m >= min(M, *m_dev) are not processed (nothing of theirs is read or written). */
    const int* perm;
    const int* m_dev;
    int rows_per_sample;
} lnx_ln_args;
int lnx_layernorm_fwd(const lnx_ln_args* args, void* stream);

typedef struct lnx_ln_bwd_args {
    int M, C;
    const void* dy;     /* rows via dy_map */
    int dy_dtype;
    int64_t lddy;
    lnx_rowmap dy_map;
    const void* x;      /* forward input, rows via x_map */
    int x_dtype;
    int64_t ldx;
    lnx_rowmap x_map;
    const float* w;
    const float* mean;
    const float* rstd;
    const float* gin;   /* optional fp32 gradient to add (rows via x_map, ldgin); may alias dx */
    int64_t ldgin;      /* a multiple of 4, as the other leading dimensions */
    void* dx;           /* rows via x_map */
    int dx_dtype;
    int64_t lddx;
    float* dw;          /* [C] += or NULL: fp32 atomics (one per workgroup without ws; with ws one per slice of workgroups of the second
                           stage), or, in deterministic mode, the whole fold of the workgroups' partial sums in ws in index order and one
                           addition (ws is then required: a call without it refuses by name) */
    float* db;
    int relu_mask;      /* 1: x is a ReLU output feeding this LN; dx *= (x > 0) */
    float* ws;          /* optional scratch for the dw/db column partials (avoids contended atomics); 16-byte aligned */
    int64_t ws_floats;  /* its capacity in floats; 2048*2*C is the most that is used */
    /* optional second output: dx2[m, :] = dx2_rowscale[m / dx2_rows_per_sample] * dx[m, :] in dx2_dtype, identity rows,
     * leading dimension lddx2.  It is the operand the NEXT branch's GEMMs read (DropPath-scaled gradient in storage
     * type, rope_2d_mhsa.py:630,643 backward), so no separate cast pass re-reads dx.  May alias dy (same dtype/ld). */
    void* dx2;
    int dx2_dtype;
    int64_t lddx2;
    const float* dx2_rowscale;
    int dx2_rows_per_sample;
    /* round 4, optional (fp8 plans with MXFP8 data gradients): the MXFP8 copy of dx2 -- e4m3 elements [M, C] with leading dimension
     * lddx2_8 (bytes = elements) and E8M0 block scales in lnx_quantize_mxfp8's layout for an [M, C] operand -- bit-identical to
     * lnx_quantize_mxfp8 of the bf16 dx2, written by the same pass, so the next branch's data-gradient product needs no quantise pass
     * over its dY.  Needs dx2 in bf16, x in fp32, C % 128 == 0, 4-byte aligned rows. */
    void* dx2_8;
    void* dx2_8_scales;
    int64_t lddx2_8;
    /* round 5.  != 0 (and ws given, dw / db wanted): the column partials stay in ws and their summation into dw / db is postponed to
     * lnx_layernorm_bwd_flush(), which sums the partials of ALL postponed calls of this host thread in one launch (up to 16; a 17th, or
     * one on another stream, flushes first).  Every pending call needs its own ws, untouched until the flush. */
    int defer;
    /* Compact rows (DropPath compaction lists, below); rows per sample = dx2_rows_per_sample, identity row maps.
     * perm / m_dev   as lnx_ln_args: dy, mean and rstd are compact (row m < min(M, *m_dev)), x, gin and dx are the sample's own rows
     *                (the gather on the x side, the scatter on the dx side).  dx rows of the samples behind the effective M are left
     *                untouched, and nothing of theirs enters dw / db.
     * dx2_inv / dx2_nkeep   the second output is compact under ANOTHER list (it is the other branch's dY): sample b's rows go to
     *                position dx2_inv[b] of dx2 and are written only if dx2_inv[b] < *dx2_nkeep; dx2_rowscale is read at b.  Without
     *                them dx2 has the samples' own rows.  With m_dev and dx2, the rows of the samples behind the effective M still get
     *                their dx2 = dx2_rowscale * gin (they take no other part), so gin is required. */
    const int* perm;
    const int* m_dev;
    const int* dx2_inv;
    const int* dx2_nkeep;
} lnx_ln_bwd_args;
int lnx_layernorm_bwd(const lnx_ln_bwd_args* args, void* stream);
/* sums the postponed column partials into their dw / db (no-op when nothing is pending; `stream` = the postponed calls' stream or NULL) */
int lnx_layernorm_bwd_flush(void* stream);
/* forgets them without summing (error paths; lnx_plan_backward does it on entry and when it fails); returns how many */
int lnx_layernorm_bwd_discard(void);

/* The launch lnx_layernorm_fwd / lnx_layernorm_bwd WOULD make for these arguments (no launch, no device work, no GPU needed; negative
 * on arguments the entry point refuses, with its message in lnx_last_error): only shapes, dtypes, leading dimensions, the alignment
 * of the pointers and WHICH optional operands are non-NULL are looked at, never the memory behind them.  The entry points take
 * their decision from the same function, so a test can prove which instantiation, grid and column-sum route a case ran on. */
enum { LNX_LN_COLS_NONE = 0 /* no dw / db wanted */, LNX_LN_COLS_ATOMICS = 1 /* one atomic per column per workgroup */,
       LNX_LN_COLS_WORKSPACE = 2 /* per-workgroup partials in ws, summed by a second stage of `slices` slices */ };
typedef struct lnx_ln_launch {
    int G;       /* lanes per row (pair mode: lanes holding float4 pairs) */
    int V;       /* float4 slots per lane */
    int pair;    /* 1: 16-byte accesses on bf16 rows (streamed operands bf16, every pointer and leading dimension 16-byte aligned) */
    int full;    /* 1: C / 4 == G * V, no partial-row code */
    int mx;      /* 1: the variant that also writes the MXFP8 copy (y8, dx2_8) */
    int grid;    /* workgroups of 256 threads */
    int cols;    /* backward: LNX_LN_COLS_*; forward: 0 */
    int slices;  /* LNX_LN_COLS_WORKSPACE: 1 or 64 slices of the second stage; otherwise 0 */
} lnx_ln_launch;
int lnx_layernorm_fwd_query(const lnx_ln_args* args, lnx_ln_launch* out);
int lnx_layernorm_bwd_query(const lnx_ln_bwd_args* args, lnx_ln_launch* out);

/* ------------------------------------------------------------------------------------
 * Depthwise 7x7 convolution, padding 3, NHWC (nn.Conv2d(C, C, 7, padding=3, groups=C),
 * blocks/convnext.py:56-58) and its two gradients.  Weights are passed as [49][C] fp32
 * (tap-major; lnx_prep_weights produces this from torch's [C,1,7,7]).
 * -----------------------------------------------------------------------------------*/
typedef struct lnx_dwconv_args {
    int B, H, W, C;       /* C % 32 == 0 */
    const void* x;        /* [B,H,W,C] */
    int x_dtype;
    const float* w49;     /* [49][C] */
    const float* bias;    /* [C] or NULL */
    int flip;             /* 1: correlate with the flipped kernel (data gradient) */
    const float* res;     /* optional fp32 [B,H,W,C] added to the output (may alias y) */
    void* y;              /* [B,H,W,C] */
    int y_dtype;
} lnx_dwconv_args;
int lnx_dwconv7_fwd(const lnx_dwconv_args* args, void* stream);
/* ... through a DropPath compaction list (lnx_drop_partition: perm [B] device, kept samples first; nkeep device int).  The kernel walks
 * the tiles of the kept samples perm[0 .. *nkeep) only, divided anew over the workgroups of the launch: the samples perm[j],
 * j >= *nkeep, are neither read nor written (their rows of y -- and with res == y their rows of the residual stream -- stay as they
 * are).  Kept samples get the bits of the call without a list. */
int lnx_dwconv7_fwd_kept(const lnx_dwconv_args* args, const int* perm, const int* nkeep, void* stream);

typedef struct lnx_dwconv_wgrad_args {
    int B, H, W, C;
    const void* x;        /* forward input [B,H,W,C] */
    int x_dtype;
    const void* dy;       /* [B,H,W,C] */
    int dy_dtype;
    float* dw;            /* torch layout [C,1,7,7], +=: one float atomic per workgroup and tap, or (deterministic mode) the workgroups'
                             partial sums through ws, folded in workgroup order and added once */
    float* db;            /* [C] += (likewise) or NULL */
    float* ws;            /* deterministic mode: scratch of lnx_dwconv7_wgrad_ws_floats(...) floats (overwritten), required; else ignored */
    int64_t ws_floats;
} lnx_dwconv_wgrad_args;
int lnx_dwconv7_wgrad(const lnx_dwconv_wgrad_args* args, void* stream);
/* ... through a DropPath compaction list, as lnx_dwconv7_fwd_kept: the sums run over the kept samples perm[0 .. *nkeep) only, x and dy
 * of the others are not read.  The deterministic route keeps one row of partial sums per walker of the launch for B samples (ws as
 * for lnx_dwconv7_wgrad), folded in walker order; a walker the list leaves without tiles adds zeros. */
int lnx_dwconv7_wgrad_kept(const lnx_dwconv_wgrad_args* args, const int* perm, const int* nkeep, void* stream);
/* floats of ws the deterministic route of lnx_dwconv7_wgrad needs for this shape and these dtypes on the current device (the launcher's
 * own grid choice: walkers x 50 C); 0 for a shape the entry point refuses */
int64_t lnx_dwconv7_wgrad_ws_floats(int B, int H, int W, int C, int x_dtype, int dy_dtype);

/* ------------------------------------------------------------------------------------
 * Attention with the reference's cos-only "2D RoPE" (SURVEY F1), global over N tokens.
 *   cos table: rope_2d_mhsa.py:56-73,114-155,397-408; q,k scaling :176-218,440-456;
 *   scores/softmax/AV :495-501.  head_dim D = C / heads is 32, 64 or 128 (64 in every shipped
 * config; the reference takes any, rope_2d_mhsa.py:76-111, scale D^-0.5).  Every struct and call
 * below that carries a head_dim takes 0 for 64, so callers written for head_dim 64 are unchanged.
 * head_dim 64 runs the resident kernels (bf16, N <= 256) or the tiled ones; 32 and 128 the tiled ones.
 * qkv is the raw output of the qkv Linear, [B*N, 3*C] with column = which*C + head*D + d
 * (:432-437); o is [B*N, C] with column = head*D + d (:501).  The first E tokens of each
 * sample are extra (CLS/meta) tokens and are not scaled by cos.
 *
 * rope_mode (every struct below carries one; 0 = what the reference computes today, so callers that zero their structs are unchanged):
 *   LNX_ROPE_COS     the pairs (x[2j], x[2j+1]) of the image tokens of q and k are multiplied by cos(theta): the reference as it runs,
 *                    whose _get_current_freqs_cis casts the complex table to float32 and drops the imaginary part (finding F1);
 *   LNX_ROPE_ROTATE  the rotation the reference's helpers define when they are handed the complex table itself -- compute_mixed_cis'
 *                    polar(1, theta) (rope_2d_mhsa.py:114-155) through apply_rotary_emb's view_as_complex product (:176-218):
 *                        x'[2j]   = x[2j] cos(theta) - x[2j+1] sin(theta)
 *                        x'[2j+1] = x[2j] sin(theta) + x[2j+1] cos(theta)          x in {q, k}
 *                    with theta[n,h,j] = t_x freqs[0,h,j] + t_y freqs[1,h,j], t_x = n % W, t_y = n / W over the N - E image tokens;
 *                    v and the E extra tokens are untouched, q is then scaled by D^-0.5 (:456) as in the cos mode.  The rotation is
 *                    applied where the cos multiply is: in the operand loaders, from the raw qkv rows, in fp32, rounded once to the
 *                    storage type -- no pre-pass over qkv, no extra activation tensor.  Backward:
 *                        dx[2j]   =  dx'[2j] cos(theta) + dx'[2j+1] sin(theta)
 *                        dx[2j+1] = -dx'[2j] sin(theta) + dx'[2j+1] cos(theta)
 *                        dtheta[n,h,j] = sum_b sum_{x in {q,k}} (dx'[2j+1] x'[2j] - dx'[2j] x'[2j+1])      (x' and dx' both after q's scale)
 *                        dfreqs[0,h,j] += sum_n t_x dtheta[n,h,j],   dfreqs[1,h,j] += sum_n t_y dtheta[n,h,j]
 *                    The backward takes t_x, t_y from the token index and grid_w (no d-cos table).  Same kernel families, same
 *                    dispatch (lnx_attn_dispatch does not look at the mode), same freq_ws size, same deferred fold.
 * -----------------------------------------------------------------------------------*/
enum { LNX_ROPE_COS = 0, LNX_ROPE_ROTATE = 1 };
/* head_dim 64 */
int lnx_rope_cos_table(const float* freqs /* [2,heads,32] */, int heads, int H, int W, float* cos_out /* [H*W,heads,32] */,
                       float* dsin_out /* optional [2][H*W,heads,32]: -t_x sin(theta), -t_y sin(theta) = d cos(theta) / d freqs[a] (what
                                          lnx_attn_bwd weights its pair gradients with) */,
                       void* stream);
/* any supported head_dim D: freqs [2,heads,D/2], cos_out [H*W,heads,D/2], dsin_out optional [2][H*W,heads,D/2] */
int lnx_rope_cos_table_hd(const float* freqs, int heads, int head_dim, int H, int W, float* cos_out, float* dsin_out, void* stream);
/* lnx_rope_cos_table_hd with the optional sin table of LNX_ROPE_ROTATE: sin_out [H*W,heads,D/2] = sin(theta), the cos table's layout
 * (entry (n * heads + h) * D/2 + j), from the same fp32 angle; NULL = lnx_rope_cos_table_hd.  dsin_out stays optional (the rotate
 * backward does not read it). */
int lnx_rope_cossin_table_hd(const float* freqs, int heads, int head_dim, int H, int W, float* cos_out, float* sin_out, float* dsin_out, void* stream);
/* The same tables for several blocks in one launch (each RoPE block owns its freqs, rope_2d_mhsa.py:397-408; a plan fills the
 * tables of all its blocks once per forward, off the main stream).  Entries as lnx_rope_cos_table_hd's arguments; one launch per
 * head_dim present. */
#define LNX_ROPE_TABLES_MAX 24
typedef struct {
    const float* freqs; /* [2,heads,D/2] */
    float* cos_out;     /* [H*W,heads,D/2] */
    float* dsin_out;    /* optional [2][H*W,heads,D/2] */
    int heads, H, W;
    int head_dim;       /* D; 0 = 64 */
    int rope_mode;      /* LNX_ROPE_COS (0) or LNX_ROPE_ROTATE: the latter needs sin_out */
    float* sin_out;     /* optional (required with LNX_ROPE_ROTATE) [H*W,heads,D/2]: sin(theta), laid out like cos_out */
} lnx_rope_table;
int lnx_rope_cos_tables(const lnx_rope_table* tables, int n, void* stream);
/* floats of lnx_attn_bwd's freqs-gradient workspace (one [2][D/2] partial per workgroup of its finest tiling): head_dim 64, and any
 * supported head_dim (0 for an unsupported one) */
int64_t lnx_attn_bwd_ws_floats(int B, int N, int heads);
int64_t lnx_attn_bwd_ws_floats_hd(int B, int N, int heads, int head_dim);

typedef struct lnx_attn_args {
    int dtype;
    int B, N, E, heads;
    const void* qkv;     /* [B*N, 3*heads*D] */
    const float* cos_tab;/* [(N-E), heads, D/2] */
    void* o;             /* [B*N, heads*D] */
    float* lse;          /* [B, heads, N] log-sum-exp of the scaled scores */
    const unsigned char* drop_mask; /* optional (training with MODEL.ATTN_DROP_RATE, rope_2d_mhsa.py:497): keep mask of the attention
                                       probabilities, one byte per (b, head, query, key), [B, heads, N, Np] with Np = N rounded up to
                                       a multiple of 64; P is multiplied by mask * drop_inv_keep AFTER the softmax normalisation.
                                       Runs the 64-row tiled kernels (the dropout-free path keeps its own instantiations). */
    float drop_inv_keep; /* 1 / (1 - ATTN_DROP_RATE) */
    int head_dim;        /* D: 32, 64 or 128; 0 = 64 */
    int rope_mode;       /* LNX_ROPE_COS (0) or LNX_ROPE_ROTATE */
    const float* sin_tab;/* LNX_ROPE_ROTATE: [(N-E), heads, D/2] sin(theta), the layout of cos_tab (lnx_rope_cossin_table_hd /
                            lnx_rope_table.sin_out); not read in the cos mode */
} lnx_attn_args;
int lnx_attn_fwd(const lnx_attn_args* args, void* stream);

typedef struct lnx_attn_bwd_args {
    int dtype;
    int B, N, E, heads;
    const void* qkv;
    const float* cos_tab;
    const void* o;
    const float* lse;
    const void* d_o;     /* [B*N, heads*D] */
    void* dqkv;          /* [B*N, 3*heads*D] */
    float* freq_ws;      /* workspace, lnx_attn_bwd_ws_floats_hd(B, N, heads, D) floats (overwritten): round 3 -- the gradient of the learnable
                            frequencies (autograd of compute_mixed_cis / apply_rotary_emb through the real part only, finding F1) is
                            reduced inside the two backward kernels to one [2][D/2] partial per workgroup; it used to be a
                            [2][B, N-E, heads, D/2] tensor read back by a separate lnx_rope_freqs_bwd.  Inside a workgroup the waves add
                            to the partial with LDS float atomics (order not fixed); in deterministic mode each wave sums into a slot
                            of its own behind the partials and the slots are folded by wave index -- the size query reports the larger
                            need while the mode is on, so allocate (and call) under the setting the query was made in.  The fold of
                            the partials into dfreqs is fixed-order in both modes. */
    float* delta;        /* workspace [B, heads, N] */
    const unsigned char* drop_mask; /* the forward's keep mask (see lnx_attn_args), or NULL */
    float drop_inv_keep;
    const float* dsin_tab; /* [2][(N-E), heads, D/2] from lnx_rope_cos_table(_hd) */
    float* dfreqs;         /* [2, heads, D/2] fp32, accumulated into (dfreqs += ...) */
    int defer_freqs;       /* 1: leave the fold of freq_ws into dfreqs to lnx_attn_bwd_flush (one launch for up to LNX_ATTN_DEFER_MAX calls of
                              this thread on this stream; freq_ws and dfreqs must stay untouched and alive until then -- a plan gives every
                              pending call its own freq_ws region and flushes at the end of each backward segment) */
    int head_dim;          /* D: 32, 64 or 128; 0 = 64 */
    int rope_mode;         /* LNX_ROPE_COS (0) or LNX_ROPE_ROTATE; the mode of the forward that produced o and lse */
    const float* sin_tab;  /* LNX_ROPE_ROTATE: the forward's sin table [(N-E), heads, D/2]; dsin_tab is then not read (may be NULL) */
    int grid_w;            /* LNX_ROPE_ROTATE: width W of the token grid the tables were built for ((N-E) = H * W): the kernels weight
                              dtheta of image token n by t_x = n % W and t_y = n / W; not read in the cos mode */
} lnx_attn_bwd_args;
#define LNX_ATTN_DEFER_MAX 16
int lnx_attn_bwd_flush(void* stream); /* folds every postponed call of this thread; refuses a stream other than theirs */
int lnx_attn_bwd_discard(void);       /* forgets them without folding (error paths); returns how many were dropped */
int lnx_attn_bwd(const lnx_attn_bwd_args* args, void* stream);
/* The same call with the size of freq_ws (floats).  Deterministic mode with image tokens (E < N): the waves' slots lie behind the
 * workgroups' partials, so the call needs to know what it was given -- less than lnx_attn_bwd_ws_floats_hd reports with the mode on
 * refuses by name, and so does lnx_attn_bwd (no size) there.  Outside the mode the size is not read. */
int lnx_attn_bwd_sized(const lnx_attn_bwd_args* args, int64_t freq_ws_floats, void* stream);
/* Compact rows (DropPath compaction lists: a list's nkeep, a device int): lnx_attn_fwd / lnx_attn_bwd_sized on buffers that are compact by
 * sample -- qkv / o / lse, d_o / dqkv / delta.  The problems of the samples b >= *nkeep are skipped before anything of theirs is read
 * or written (their slots may hold anything), their slots of freq_ws are neither written nor folded into dfreqs (immediate and
 * postponed fold alike: nkeep must stay valid until the flush).  Not together with drop_mask.  nkeep == NULL: the plain calls. */
int lnx_attn_fwd_compact(const lnx_attn_args* args, const int* nkeep, void* stream);
int lnx_attn_bwd_compact(const lnx_attn_bwd_args* args, const int* nkeep, int64_t freq_ws_floats, void* stream);

/* Which kernel family lnx_attn_fwd / lnx_attn_bwd take (host-side bookkeeping, no device work; the forward and the backward of one
 * call take the same one): the boundary tests use it to prove that a sequence length ran on the kernels it is meant to cover.
 *   resident (bf16, head_dim 64, no dropout mask, N <= 256): 4 waves at N <= 64, 8 waves beyond.  Their backward is ONE kernel per
 *     call at N <= 224 (every operand staged in LDS once for both the dq and the dk / dv phase; 4 waves at N <= 64, 16 beyond) and the
 *     dq / dk-dv pair of 4- / 8-wave kernels at 225..256 (four operand images no longer fit the LDS) and, at every resident N, with
 *     LNX_ATTN_BWD_SPLIT in the environment (read per call: the A/B switch).  The family reported is the same either way, and so are
 *     dqkv and delta bit for bit (the rotating mode included);
 *   tiled, 4 waves (64-row tiles): fp32; any call with a dropout mask; bf16 head_dim 32; bf16 head_dim 64 / 128 at N <= 128 where
 *     the resident kernels do not take it, and at every N with LNX_ATTN_NW=4 in the environment (read once per process);
 *   tiled, 8 waves (128-row tiles): bf16 head_dim 128 at N > 128; bf16 head_dim 64 at N > 256, and at N > 128 with LNX_ATTN_TILED
 *     in the environment (read per call: no resident kernels).
 * lnx_attn_dispatch(): the family a launch with these arguments would take now (head_dim 0 = 64; has_drop_mask != 0: a dropout
 *   mask is passed); negative for a dtype, N or head_dim the entry points refuse.  The entry points decide with the same function.
 * lnx_last_attn_kernel(): family of the most recent lnx_attn_fwd / lnx_attn_bwd launch of this process (any stream), 0 before the first.
 * lnx_last_attn_bwd_launches(): attention kernels the most recent lnx_attn_bwd launched (the freqs fold not counted): 1 for the
 *   one-kernel resident backward, 2 for every pair; 0 before the first lnx_attn_bwd. */
enum { LNX_ATTN_KERNEL_NONE = 0, LNX_ATTN_KERNEL_RES4 = 1 /* resident, 4 waves */, LNX_ATTN_KERNEL_RES8 = 2 /* resident, 8 waves */,
       LNX_ATTN_KERNEL_TILED4 = 3 /* tiled, 64-row tiles */, LNX_ATTN_KERNEL_TILED8 = 4 /* tiled, 128-row tiles */ };
int lnx_attn_dispatch(int dtype, int N, int head_dim, int has_drop_mask);
int lnx_last_attn_kernel(void);
int lnx_last_attn_bwd_launches(void);

/* ------------------------------------------------------------------------------------
 * Small data-movement / elementwise kernels of the path
 * -----------------------------------------------------------------------------------*/
/* stem im2col: x fp32 NCHW [B,Cin,H,W] -> patches [B*(H/4)*(W/4), ldp] of T with column
 * k = c*16 + kh*4 + kw (torch conv weight order), zero padded to ldp (mFormerV1.py:146) */
int lnx_im2col_stem(const float* x, int B, int Cin, int H, int W, void* patches, int dtype, int ldp, void* stream);

/* The whole stem in one launch (bf16 compute type; csrc/stem.hip): nn.Conv2d(in_chans, dims[0], 4, 4) + bias, output rounded
 * to bf16 as under autocast, then LayerNorm(dims[0], eps, "channels_first") -- mFormerV1.py:145-148.  Writes the fp32
 * normalised rows `y` and, when asked (training plans), what the backward reads: the bf16 patch matrix [M, 64] of
 * lnx_im2col_stem, the bf16 pre-norm tensor [M, Cout] and the row statistics.  lnx_stem_fwd_ok() tells whether the geometry is
 * covered (Cin <= 4, H and W multiples of 4, Cout in {96, 128, 192, 256}); otherwise im2col + lnx_gemm_nt + lnx_layernorm_fwd. */
typedef struct lnx_stem_args {
    const float* x;      /* [B, Cin, H, W] fp32 */
    const void* w;       /* bf16 [Cout, 64], column k = c*16 + kh*4 + kw */
    const float* bias;   /* [Cout] */
    const float* ln_w;   /* [Cout] */
    const float* ln_b;   /* [Cout] */
    void* patches;       /* bf16 [M, 64] or NULL */
    void* pre;           /* bf16 [M, Cout] or NULL */
    float* y;            /* fp32 [M, Cout], M = B * H/4 * W/4 */
    float* mean;         /* [M] or NULL (with rstd) */
    float* rstd;
    int B, Cin, H, W, Cout;
    float eps;
} lnx_stem_args;
int lnx_stem_fwd_ok(int dtype, int Cin, int H, int W, int Cout);
int lnx_stem_fwd(const lnx_stem_args* args, void* stream);

/* Input gradient of the stem convolution (lnx_version 121; csrc/stem.hip): the transpose of nn.Conv2d(Cin, Cout, 4, 4),
 *     dx[b, c, 4i + kh, 4j + kw] = sum over o of dy[m, o] * w[o, c*16 + kh*4 + kw],   m = (b * H/4 + i) * W/4 + j,
 * what F.conv_transpose2d(dy as NCHW, weight, stride = 4) gives.  dy is the gradient at the convolution's output (the stem LayerNorm
 * backward's dx), rows of ldy elements of which the first Cout count (whatever the padding holds is never read); w is the operand
 * arena's [Cout, 64] copy the forward reads (columns >= Cin * 16 are never read).  EVERY element of dx is written exactly once (one
 * contributor per element, no atomics, nothing to pre-zero), as 16-byte stores: in the MFMA result layout a lane holds the four kw of
 * one (patch, c, kh), and the sixteen patches of a tile are neighbours along W, so a store instruction writes 256 contiguous bytes per
 * (c, kh) row without a pass through LDS.
 *   LNX_BF16: v_mfma_f32_16x16x32_bf16, fp32 accumulation.   LNX_F32: v_mfma_f32_16x16x4_f32, an exact fp32 FMA chain (strict parity).
 * lnx_stem_dgrad_ok mirrors lnx_stem_fwd_ok (Cin <= 4, H and W multiples of 4, Cout in {96, 128, 192, 256}) for both dtypes;
 * LNX_NO_FUSED_STEM_DGRAD in the environment makes it answer 0 (A/B against the fallback).  Every other geometry:
 * lnx_gemm_nt(dy, transposed weight copy [Cin * 16, Cout]) -> fp32 [M, Cin * 16], then lnx_col2im_stem. */
typedef struct lnx_stem_dgrad_args {
    int dtype;           /* LNX_BF16 or LNX_F32: the type of dy and w */
    int B, Cin, H, W, Cout;
    const void* dy;      /* T [M, ldy], M = B * H/4 * W/4; 16-byte aligned rows */
    int64_t ldy;
    const void* w;       /* T [Cout, 64], column k = c*16 + kh*4 + kw */
    float* dx;           /* fp32 [B, Cin, H, W], 16-byte aligned */
} lnx_stem_dgrad_args;
int lnx_stem_dgrad_ok(int dtype, int Cin, int H, int W, int Cout);
int lnx_stem_dgrad(const lnx_stem_dgrad_args* args, void* stream);
/* The inverse of lnx_im2col_stem: patches [B*(H/4)*(W/4), ldp] of T, column k = c*16 + kh*4 + kw  ->  dx fp32 NCHW [B, Cin, H, W],
 * every element written once (columns >= Cin * 16 of a patch row are not read). */
int lnx_col2im_stem(const void* patches, int dtype, int ldp, int B, int Cin, int H, int W, float* dx, void* stream);

/* out[m, :] = rowscale[m / rows_per_sample] * in[map(m), :]   (fp32 in, T or fp32 out) */
int lnx_scale_cast(const float* in, int64_t ldin, lnx_rowmap in_map, const float* rowscale, int rows_per_sample, void* out,
                   int out_dtype, int64_t ldout, int M, int C, void* stream);

/* ------------------------------------------------------------------------------------
 * DropPath compaction lists.  A DropPath multiplier (drop_path.py:29-33) is 1 / keep or exactly 0 per sample; for a sample with 0 the
 * branch's forward result is its input and its dY rows are 0, so none of the branch's kernels has anything to compute for it.  The
 * multipliers are drawn on the device, so the lists are built there too (no host synchronisation), and every consumer reads the
 * kept count from device memory.
 *
 * lnx_drop_partition: scales is [n_calls][B]; for every call c (with call_mask[c] != 0 when the HOST array call_mask is given) one
 * launch writes that call's list, LNX_DROP_LIST_INTS(B) ints at lists + c * LNX_DROP_LIST_INTS(B):
 *   [0]            nkeep  = number of samples whose multiplier is not exactly 0.0 (any other value, NaN included, counts as kept)
 *   [1]            m_eff  = nkeep * rows_per_sample[c]   (rows_per_sample: HOST array or NULL = 1): what `m_dev` arguments point at
 *   [2, 2 + B)     perm   : stable partition of 0 .. B-1 -- the kept samples in ascending order, then the dropped ones in ascending order
 *   [2 + B, 2+2B)  inv    : inv[perm[j]] = j, a sample's position under this list
 * COMPACT ROWS of a call: compact row m' stands for sample perm[m' / rows_per_sample], token m' % rows_per_sample; rows m' < m_eff are
 * the kept samples' rows, rows >= m_eff are nobody's: a kernel with an `m_dev` argument neither reads them into a result nor writes them
 * (they may hold anything, NaN included).
 * -----------------------------------------------------------------------------------*/
#define LNX_DROP_LIST_INTS(B) (2 * (B) + 2)
#define LNX_DROP_PARTITION_MAX 64 /* calls per launch (more calls: more launches) */
int lnx_drop_partition(const float* scales, int n_calls, int B, const unsigned char* call_mask, const int* rows_per_sample, int* lists, void* stream);
/* lnx_scale_cast with compact output rows: out[m', :] = rowscale[b] * in[b * rows_per_sample + m' % rows_per_sample, :] with
 * b = perm[m' / rows_per_sample], for m' < min(M, *m_dev); M = B * rows_per_sample.  rowscale may be NULL (1). */
int lnx_scale_cast_compact(const float* in, int64_t ldin, const float* rowscale, int rows_per_sample, const int* perm, const int* m_dev, void* out,
                           int out_dtype, int64_t ldout, int M, int C, void* stream);

/* dst rows of the samples a list drops = src rows, bit for bit (the residual forms with perm leave them untouched): rows
 * perm[j] * rows_per_sample + t for j >= *nkeep, C fp32 columns, leading dimension ld for both. */
int lnx_copy_dropped_rows(const float* src, float* dst, int64_t ld, const int* perm, const int* nkeep, int B, int rows_per_sample, int C, void* stream);

/* A/B switch of the DropPath compaction inside lnx_plan_forward / lnx_plan_backward, process-wide: on = 0 / 1, or -1 = back to the
 * environment (LNX_DROP_COMPACT, on unless it is 0).  Returns the previous setting (-1, 0 or 1).  Read by every lnx_plan_forward; a
 * backward follows its forward's choice.  lnx_drop_compact_branches(): RoPE-block branches that ran a forward on compact rows since
 * the library was loaded (the tests' proof of which path a plan took, like lnx_last_nt_kernel). */
int lnx_set_drop_compact(int on);
int64_t lnx_drop_compact_branches(void);
/* The conv blocks' share (blocks that run fused with the LayerNorm inside): LNX_DROP_COMPACT_CONV=0 keeps them on full rows while the
 * RoPE blocks compact (read by every lnx_plan_forward).  lnx_drop_compact_conv_blocks(): conv blocks that ran a forward on compact
 * rows since the library was loaded; lnx_drop_compact_branches() keeps counting RoPE branches only. */
int64_t lnx_drop_compact_conv_blocks(void);
/* A/B switch of the CLS-only last RoPE block inside lnx_plan_forward / lnx_plan_backward, process-wide: on = 0 / 1, or -1 = back to the
 * environment (LNX_LAST_CLS, on unless it is 0).  Returns the previous setting (-1, 0 or 1).  norm_2 reads only the CLS row of the
 * stage-4 output (mFormerV1.py:509-527), so the last stage-4 block runs LayerNorm 1, qkv and attention on all rows and proj, LayerNorm 2,
 * fc1 and fc2 -- forward, data and weight gradients -- on the batch's CLS rows alone; the other rows of that block's xmid and output are
 * never written.  Same arithmetic on fewer rows: logits, loss and gradients are what the full block gives up to summation order and the
 * kernel family a product of M = batch rows dispatches to.  Read by every lnx_plan_forward; a backward follows its forward's choice.
 * fp8 plans and plans with dropout masks keep the full block.  lnx_last_cls_blocks(): block forwards that took the path since the
 * library was loaded. */
int lnx_set_last_cls(int on);
int64_t lnx_last_cls_blocks(void);

/* LayerScale+DropPath backward of a ConvNeXt block branch (blocks/convnext.py:82-86):
 * dz = rowscale * gamma * g  (T),  dgamma[c] += sum_m rowscale * g * z */
int lnx_layerscale_bwd(const float* g, const void* z, int dtype, const float* gamma, const float* rowscale,
                       int rows_per_sample, void* dz, float* dgamma, int M, int C, void* stream);

/* Round 4.  The LayerScale gradient of a ConvNeXt block WITHOUT the saved pwconv2 output z (blocks/convnext.py:80-83: x = gamma * z,
 * z = act . W2^T + b2).  dgamma[c] = sum_m rs g[m, c] z[m, c] = sum_k W2[c, k] S[c, k] + b2[c] T[c] with S = (rs g)^T act and
 * T = colsum(rs g) -- and the pwconv2 weight / bias gradients are gamma[c] S[c, :] and gamma[c] T[c].  So the weight-gradient product
 * runs on dY = rs g (lnx_convmlp_bwd_args.dz_plain) into ZEROED scratch s [C, K] / t [C] instead of the gradient buffers, and one launch does
 *     dw[c, :] += gamma[c] s[c, :]      db[c] += gamma[c] t[c]      dgamma[c] += sum_k w[c, k] s[c, k] + b[c] t[c]
 * with w, b the fp32 master weight / bias of pwconv2.  No division by gamma (gamma = 0 is an ordinary value), nothing about what the
 * gradient buffers held before.  The forward then no longer writes z (1.4 GB / step at mFormerV1_sm, batch 256) and the backward kernels
 * neither read it nor carry the column sums. */
int lnx_layerscale_apply_wgrad(const float* s, const float* t, int64_t lds, const float* w, const float* b, int64_t ldw, const float* gamma, float* dw, float* db,
                               int64_t lddw, float* dgamma, int C, int K, void* stream);

/* Dropout of the RoPE blocks' Linear outputs (MODEL.DROP_RATE: blocks/mlp.py:61-66 `self.drop`, rope_2d_mhsa.py:503
 * `proj_drop`), with the keep mask drawn by the caller (one byte per element, 1 = keep):
 *   lnx_dropout_mul       x[m, c] = mask[m, c] ? x[m, c] * inv_keep : 0            (in place; T or fp32; C % 8 == 0)
 *   lnx_dropout_residual  out[m, c] = res[m, c] + rowscale[m / rps] * (mask[m, c] ? z[m, c] * inv_keep : 0)   (z of T, fp32 res / out)
 * They are separate passes, not epilogue forms: no shipped configuration trains with dropout, the default path stays as it is. */
int lnx_dropout_mul(void* x, int dtype, const unsigned char* mask, float inv_keep, int M, int C, void* stream);
int lnx_dropout_residual(const void* z, int z_dtype, const unsigned char* mask, float inv_keep, const float* rowscale, int rows_per_sample,
                         const float* res, float* out, int M, int C, void* stream);

/* out[map(m), :] = vec[:]  for m in [0, M)   (CLS token expand, mFormerV1.py:448,487) */
int lnx_fill_rows(const float* vec, float* out, int64_t ldout, lnx_rowmap map, int M, int C, void* stream);
/* out[c] += sum_m in[map(m), c]   (fp32 atomics) */
/* lnx_layerscale_bwd with scratch for the deterministic mode: ws holds lnx_layerscale_bwd_ws_floats(M, C) floats (the workgroups'
 * dgamma partial sums, folded in workgroup order and added to dgamma once).  Outside the mode ws is ignored; inside it
 * lnx_layerscale_bwd (no scratch) refuses by name.  The size query returns 0 for a shape the entry point refuses. */
int lnx_layerscale_bwd_ws(const float* g, const void* z, int dtype, const float* gamma, const float* rowscale, int rows_per_sample, void* dz,
                          float* dgamma, int M, int C, float* ws, int64_t ws_floats, void* stream);
int64_t lnx_layerscale_bwd_ws_floats(int M, int C);
/* (deterministic mode: lnx_colsum_rows and lnx_agg2_bwd run ONE workgroup over all rows / elements -- one contributor per output,
 * no scratch.  That is sized for their callers in the plan (M = batch rows); a caller with a large M gets a serial kernel there.) */
int lnx_colsum_rows(const float* in, int64_t ldin, lnx_rowmap map, float* out, int M, int C, void* stream);

/* aggregate = Conv1d(2,1,1) over [cls_1, cls_2] (mFormerV1.py:322,515-523):
 * out = w[0]*a + w[1]*b + bias[0] */
int lnx_agg2_fwd(const float* a, const float* b, const float* w2, const float* bias1, float* out, int M, int C, void* stream);
/* da = w0*dout, db = w1*dout, dw[0] += <dout,a>, dw[1] += <dout,b>, dbias += sum(dout) */
int lnx_agg2_bwd(const float* dout, const float* a, const float* b, const float* w2, float* da, float* db_, float* dw2,
                 float* dbias1, int M, int C, void* stream);

/* meta [B, width] fp32 -> T [B, 16] holding columns [off, off+dim) zero padded */
int lnx_pack_meta(const float* meta, int width, int off, int dim, void* out, int dtype, int B, void* stream);

/* ------------------------------------------------------------------------------------
 * Metadata-head chains, one launch per direction (round 5).  Replaces, per metadata component and RoPE stage, the chain
 *     Linear(d, C) -> ReLU -> LayerNorm(C) -> ResNormLayer:  x + LN2(ReLU(W2 . LN1(ReLU(W1 . x))))
 * of /root/reference/linnaeus/models/mFormerV1.py:282-311 and normalization/res_norm_layer.py:23-30 (eps 1e-5 everywhere),
 * and its autograd backward -- until round 4 seven GEMM / LayerNorm launches per head forward and thirteen backward.
 * fp32 storage and fp32 matrix-core arithmetic whatever the plan's dtype (M = batch rows: the cost is launches, not FLOPs).
 * One workgroup takes 16 batch rows through the whole chain; every head passed in one call shares one launch (four per launch).
 * All buffers are the caller's (no allocation, no host synchronisation); rows are 16-byte aligned.
 * ------------------------------------------------------------------------------------ */
typedef struct lnx_meta_head_args {
    int B, C;                 /* batch rows; width of the RoPE stage this head feeds: lnx_meta_heads_supported(C), i.e. C / 128 in {1, 2, 3, 4, 6, 8} */
    int dim, off;             /* this component's input width (1..16) and its first column in `meta` */
    const float* meta;        /* [B, meta_width] */
    int meta_width;
    float eps;                /* LayerNorm eps (the reference: 1e-5) */
    const float* w0;          /* [C, ldw0], columns >= dim zero (the operand arena's copy of `.0.weight`); ldw0 >= 16 */
    int ldw0;
    const float *b0, *ln0_w, *ln0_b;   /* `.0.bias`, `.2.weight`, `.2.bias` */
    const float* w1;          /* [C, ldw1]  `.3.w1.weight` */
    int ldw1;
    const float *b1, *ln1_w, *ln1_b;   /* `.3.w1.bias`, `.3.norm_fn1.*` */
    const float* w2;          /* [C, ldw2]  `.3.w2.weight` */
    int ldw2;
    const float *b2, *ln2_w, *ln2_b;   /* `.3.w2.bias`, `.3.norm_fn2.*` */
    /* activations kept for the backward (also the chain's own scratch: always required) */
    float* t0;                /* [B, 16]  the metadata slice, zero padded */
    float *h0, *x, *h1, *n1, *h2;      /* [B, C] each: ReLU outputs h0 / h1 / h2, LayerNorm outputs x / n1 */
    float *m0, *r0, *m1, *r1, *m2, *r2; /* [B] each: mean / rstd of the three LayerNorms */
    /* output: row b goes to tok[b * tok_row_stride + tok_row_offset .. + C) (the token matrix of the stage: stride N C, offset (1 + m) C) */
    float* tok;
    int64_t tok_row_stride, tok_row_offset;
} lnx_meta_head_args;
/* 1 when the one-launch chain carries this width (heads of one call may have different widths: a launch per run of equal ones) */
int lnx_meta_heads_supported(int C);
int lnx_meta_heads_fwd(const lnx_meta_head_args* heads, int n_heads, void* stream);

typedef struct lnx_meta_head_bwd_args {
    int B, C, dim;
    const float* g;           /* token-matrix gradient: row b at g[b * g_row_stride + g_row_offset .. + C) */
    int64_t g_row_stride, g_row_offset;
    const float* w1t;         /* transposed copies [C_in, ld]: w1t[i][o] = w1[o][i] */
    int ldw1t;
    const float* w2t;
    int ldw2t;
    const float *ln0_w, *ln1_w, *ln2_w;
    const float *t0, *h0, *x, *h1, *n1, *h2, *m0, *r0, *m1, *r1, *m2, *r2;   /* what the forward left */
    float *dp2, *dp1, *dp0;   /* [B, C] scratch each: gradients wrt the three Linear outputs (before the ReLU) */
    float* part;              /* scratch, lnx_meta_heads_bwd_part_floats(B, C) floats: per-row-group column sums of the LayerNorm gradients */
    /* gradients, ACCUMULATED (+=) in a fixed order (no atomics): */
    float* d_w0;              /* [C, dim] (torch layout of `.0.weight`) */
    float *d_b0, *d_ln0_w, *d_ln0_b;
    float* d_w1;              /* [C, C] */
    float *d_b1, *d_ln1_w, *d_ln1_b;
    float* d_w2;              /* [C, C] */
    float *d_b2, *d_ln2_w, *d_ln2_b;
} lnx_meta_head_bwd_args;
int64_t lnx_meta_heads_bwd_part_floats(int B, int C);
/* two launches per (up to four) heads: the data-gradient chain, then every weight / bias / LayerNorm gradient of those heads */
int lnx_meta_heads_bwd(const lnx_meta_head_bwd_args* heads, int n_heads, void* stream);

/* Gradient with respect to the metadata itself (lnx_version 121): for every head of the call
 *     dmeta[b, off + j]  (+)=  sum over o of dp0[b, o] * w0[o, j],     j < dim,
 * dp0 = the gradient at the first Linear's output, before the ReLU mask is needed again (lnx_meta_head_bwd_args.dp0 of the one-launch
 * chain, or the launch-by-launch path's last LayerNorm-backward output), w0 = the operand arena's copy of `.0.weight`.  One launch for up
 * to LNX_MAX_META heads; fp32 throughout; one wave per (row, head) sums over o in a fixed order (each lane its stride-64 share in
 * ascending order, then a fixed butterfly), so the result is the same bits run to run with or without the deterministic mode.  No atomics:
 * the heads of ONE call must cover disjoint column ranges (the components of one RoPE stage do); a component's two contributions -- one
 * per RoPE stage -- come from two calls on one stream, the first with accumulate = 0 (write), the second with accumulate = 1 (add).
 * Any width C >= 1 (the one-launch chain's widths and the wider ones of the launch-by-launch path alike). */
typedef struct lnx_meta_input_grad_args {
    int B, C;            /* batch rows; width of the head (columns of dp0, rows of w0) */
    int dim, off;        /* the component's input width (1..16) and its first column in dmeta */
    const float* dp0;    /* [B, lddp0] */
    int64_t lddp0;
    const float* w0;     /* [C, ldw0], ldw0 >= dim */
    int ldw0;
} lnx_meta_input_grad_args;
int lnx_meta_input_grad(const lnx_meta_input_grad_args* heads, int n_heads, float* dmeta, int meta_width, int accumulate, void* stream);

/* Per-step parameter preparation: cast fp32 master parameters into the T-typed operand
 * arena the GEMMs read (plus transposed copies for the data-gradient GEMMs and the
 * tap-major depthwise weights).  `descs` is a DEVICE array built by the caller. */
enum { LNX_PREP_CAST = 0, LNX_PREP_CONV_PERM = 1, LNX_PREP_DW49 = 2 };
typedef struct lnx_prep_desc {
    const float* src;
    void* dst;        /* [rows, ld] of T (DW49: fp32 [49][C]) */
    void* dst_t;      /* optional transposed copy [cols_out, ld_t] of T, or NULL */
    int rows, cols;   /* source logical shape [rows, cols]; CONV_PERM: cols = C*P */
    int ld, ld_t;
    int P;            /* CONV_PERM: kernel positions per channel (4 for 2x2) */
    int mode;
    int block_start;  /* first workgroup index of this tensor (exclusive prefix sums) */
} lnx_prep_desc;
int lnx_prep_weights(const lnx_prep_desc* descs_dev, int ndesc, int total_blocks, int dtype, void* stream);
/* number of workgroups lnx_prep_weights needs for one tensor */
int lnx_prep_blocks(int rows, int ld, int cols, int ld_t, int has_t);



/* ------------------------------------------------------------------------------------
 * Soft-label cross entropy, forward and logits gradient in one launch ("loss on device").
 * Replaces TaxonomyAwareLabelSmoothingCE.forward (loss/taxonomy_label_smoothing.py:233-405):
 *   loss[b] = class_weight[t_b] * -sum_c soft[t_b, c] * log_softmax(logits[b])[c],  0 where t_b == ignore_index
 * and, with soft == NULL, torch.nn.functional.cross_entropy(..., label_smoothing = smoothing) per sample.
 *   dlogits[b, c] = scale * row_scale[b] * class_weight[t_b] * (softmax(logits[b])[c] * sum_c soft[t_b, c] - soft[t_b, c])
 *   loss_sum     += scale * sum_b row_scale[b] * loss[b]                (atomic; caller zeroes it)
 * `form` selects how the row S of `loss = cw * (lse * sum S - sum S x)`, `dlogits = coef * (exp(x - lse) * sum S - S)` is formed:
 *   LNX_CE_FORM_DEFAULT    S = soft[t_b, :], or with soft == NULL smoothing / C everywhere plus 1 - smoothing at t_b (torch's label smoothing)
 *   LNX_CE_FORM_OFF_TARGET S = 1 - smoothing at t_b, smoothing / (C - 1) elsewhere (LabelSmoothingCrossEntropy, loss/basic_loss.py:95-185);
 *                          soft == NULL, C >= 2; smoothing == 0 gives the bits of the default form
 *   LNX_CE_FORM_SOFT_ROW   S = soft_target[b, :] (SoftTargetCrossEntropy, loss/basic_loss.py:188-228): sum S is summed, never assumed to be 1, and
 *                          cw = sum_c soft_target[b, c] * class_weight[c].  target is not read; no soft matrix, no ignore_index.  A row whose
 *                          sum is not finite (NaN or infinite entries) gives a NaN loss and a zero gradient row
 *   LNX_CE_FORM_TAXONOMY   (lnx_version 115) S = row t_b of the taxonomy smoothing matrix, formed per column from two small tables instead of
 *                          being read from a [C, C] matrix (the table form of TaxonomyAwareLabelSmoothingCE; see lnx_taxonomy_rows below):
 *                            S[c] = tax_val[t_b, 0] if c == t_b, else tax_val[t_b, k*],  k* = the first k in 1..tax_depth with
 *                            tax_anc[k-1, c] == tax_anc[k-1, t_b] >= 0, or tax_depth + 1 if there is none
 *                          soft == NULL, smoothing == 0, target required; sum S is summed like any other row.  Everything else (a target
 *                          outside [0, C), ignore_index, class_weight, sum_ws) is as in the default form, and with the tables of a matrix
 *                          (lnx_taxonomy_rows) the same logits give the same bits as with soft = that matrix
 * sizeof(lnx_softce_args) is 168 bytes with the taxonomy fields (lnx_softce_multi passes 8 of them by value: 1344 bytes of the 4 KB
 * kernel-argument segment).
 * -----------------------------------------------------------------------------------*/
enum { LNX_CE_FORM_DEFAULT = 0, LNX_CE_FORM_OFF_TARGET = 1, LNX_CE_FORM_SOFT_ROW = 2, LNX_CE_FORM_TAXONOMY = 3 };
#define LNX_TAX_MAX_DEPTH 8 /* levels above the task's own that the taxonomy tables may hold */
typedef struct lnx_softce_args {
    int B, C;
    const float* logits;       /* [B, ld] fp32 */
    int64_t ld;
    const int64_t* target;     /* [B] class indices (not read, may be NULL, with LNX_CE_FORM_SOFT_ROW) */
    const float* soft;         /* [C, C] soft-label matrix (rows sum to 1) or NULL = one-hot */
    float smoothing;           /* soft == NULL only: uniform label smoothing epsilon */
    const float* class_weight; /* [C] or NULL */
    int64_t ignore_index;      /* < 0: none */
    const float* row_scale;    /* [B] or NULL: per-sample multiplier of the gradient / of loss_sum */
    float scale;               /* global multiplier (e.g. task_weight / B) */
    float* loss;               /* [B] per-sample losses or NULL */
    float* loss_sum;           /* scalar accumulator or NULL (+=: float atomics, or the fold through sum_ws in deterministic mode) */
    float* dlogits;            /* [B, ldd] or NULL */
    int64_t ldd;
    int form;                  /* LNX_CE_FORM_*; 0 = the two forms above */
    const float* soft_target;  /* LNX_CE_FORM_SOFT_ROW: [B, ldt] per-sample rows; NULL otherwise */
    int64_t ldt;               /* >= C */
    /* added (lnx_version 115) in front of sum_ws, which stays the last field: the tables of LNX_CE_FORM_TAXONOMY; zero-filled with any
     * other form: the call as before */
    const int32_t* tax_anc;    /* [tax_depth, C] level-major: tax_anc[k-1, c] = index at level + k of the k-th ancestor of class c, -1 once the
                                  chain has ended; may be NULL when tax_depth == 0 */
    const float* tax_val;      /* [C, tax_depth + 2]: the diagonal value, one value per height 1..tax_depth, one for disconnected classes */
    int tax_depth;             /* 0..LNX_TAX_MAX_DEPTH */
    float* sum_ws;             /* [B] scratch or NULL.  Deterministic mode with loss_sum: required -- the rows' terms go here and are folded
                                  into loss_sum in row order (otherwise one float atomic per row, in any order); ignored outside the mode */
} lnx_softce_args;
int lnx_softce(const lnx_softce_args* args, void* stream);
/* n <= LNX_SOFTCE_MAX_TASKS independent argument sets (the tasks of the multi-task criterion: train.py's per-task loop over
 * `criteria`, loss/hierarchical_loss.py:130-190) in ONE launch */
#define LNX_SOFTCE_MAX_TASKS 8
int lnx_softce_multi(const lnx_softce_args* args, int n, void* stream);

/* Rows of the dense [C, C] matrices that the taxonomy tables stand for (lnx_version 115): the device replacement of
 * build_taxonomy_smoothing_matrix (loss/taxonomy_label_smoothing.py:30-128) and of TaxonomyTree.build_distance_matrix
 * (utils/taxonomy/taxonomy_tree.py:364-381) for whoever still wants the matrix, or a few rows of it.  ONE launch, one workgroup per row:
 *   r = rows ? rows[i] : i;   k(c) = 0 if c == r, else the k* of LNX_CE_FORM_TAXONOMY above (1..depth, or depth + 1 = disconnected)
 *   what == 0: out[i, c] = val[r, k(c)]                                   (soft labels)
 *   what == 1: out[i, c] = 0 if c == r, 2 k(c), +inf where disconnected   (distances; val is not read and may be NULL)
 * for c < C; columns C..ldo-1 of out are not written.  A row index outside [0, C) gives a row of NaN. */
typedef struct lnx_taxonomy_rows_args {
    int C, depth;          /* depth in 0..LNX_TAX_MAX_DEPTH */
    const int32_t* anc;    /* [depth, C] level-major, -1 = the chain has ended; may be NULL when depth == 0 */
    const float* val;      /* [C, depth + 2] */
    const int64_t* rows;   /* [n] row indices, or NULL = 0..n-1 */
    int n;
    float* out;            /* [n, ldo] fp32 */
    int64_t ldo;           /* >= C */
    int what;              /* 0 = soft labels, 1 = distances */
} lnx_taxonomy_rows_args;
int lnx_taxonomy_rows(const lnx_taxonomy_rows_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * GPU-side batch mixing of the collate step: selective Mixup / CutMix and the metadata chunk pick.
 * Replaces linnaeus/aug/gpu/selective_mixup.py:140-230,420-560 and selective_cutmix.py:200-260 (fp32 batches).
 *   mode 0  out[b] = lam x[b] + (1-lam) x[perm[b]]                          (mixup of images / soft targets)
 *   mode 1  out[b] = x[b] with the box [h0,h1) x [w0,w1) taken from x[perm[b]] where valid[b]      (cutmix images)
 *   mode 2  out[b] = valid[b] ? lam x[b] + (1-lam) x[perm[b]] : x[b]                               (cutmix targets)
 * -----------------------------------------------------------------------------------*/
typedef struct lnx_mix_args {
    const float* x;             /* [B, row] */
    const int64_t* perm;        /* [B] partner index (perm[b] == b: unchanged) */
    const unsigned char* valid; /* [B] or NULL (= all valid) */
    float* out;                 /* [B, row], must not alias x */
    int B;
    int64_t row;                /* elements per sample, multiple of 4; mode 1: C*H*W */
    int H, W;                   /* mode 1 only */
    float lam;
    int h0, h1, w0, w1;         /* mode 1 only */
    int mode;
} lnx_mix_args;
int lnx_mix_rows(const lnx_mix_args* args, void* stream);
/* metadata [B, D] with validity mask [B, D] (bytes): per chunk (bounds_dev = device int[2*nchunk] of [start, end)) a chunk
 * with any zero entry counts as absent; both present -> own if pick[b] < 0.5 else the partner's; one present -> it; none ->
 * zeros and an all-false mask */
int lnx_mix_meta(const float* aux, const unsigned char* mask, const int64_t* perm, const float* pick, const int* bounds_dev, int nchunk, int B, int D,
                 float* out_aux, unsigned char* out_mask, void* stream);

/* Scheduled metadata masking of the collate step, full and partial, in ONE launch.  Replaces the per-sample loop of
 * linnaeus/h5data/h5dataloader.py:709-940 (with _apply_partial_mask, :366-482, and ops_schedule.py:628-650), the component
 * statistics of :1677-1801 and the evaluation-time zeroing of validation.py:174-175,192,428-489.
 *   training form (draws != NULL), per row b:
 *     full     if draws[0][b] < p_full
 *     partial  else if partial_on && draws[1][b] < p_partial, with combination k = combo_idx ? combo_idx[b]
 *              : the first k with draws[2][b] < combo_thr[k] (the host makes combo_thr[ncombo-1] = 1); k outside [0, ncombo): none
 *   evaluation form (draws == NULL; combo_idx NULL, p_full 0, partial_on 0): every row is full if row_full, else takes row_bits
 *   a column is cleared (aux 0, mask byte 0) when its row is full or when a component holding it has its bit in the row's
 *   bitmask; columns outside every component are cleared only by a full row; every other element copies through.
 * Comparisons are strict, as in the reference: p = 0 masks nothing, p = 1 masks every draw of [0, 1).
 * out_aux / out_mask may be the inputs (in place) or distinct buffers; a NULL output is not written (out_aux NULL: aux may be
 * NULL too; out_mask and counts NULL: mask may be NULL).  counts[0] += full rows, counts[1] += rows with a combination,
 * counts[2 + c] += rows whose OUTPUT mask is nonzero over all of component c (integer atomics; the caller zeroes counts).
 * With nothing to mask the call is the statistics pass alone. */
#define LNX_META_MASK_MAX_COMPONENTS 32
typedef struct lnx_meta_mask_args {
    const float* aux;              /* [B, D] fp32 */
    const unsigned char* mask;     /* [B, D] bytes, nonzero = valid */
    float* out_aux;                /* [B, D] or NULL */
    unsigned char* out_mask;       /* [B, D] or NULL */
    int B, D;
    const int* bounds;             /* device int[2 * ncomp] of [start, end), as lnx_mix_meta takes; the kernel never indexes past D */
    int ncomp;                     /* <= LNX_META_MASK_MAX_COMPONENTS */
    int ncombo;
    const unsigned int* combo_bits; /* device [ncombo]: bit c = component c belongs to the combination */
    const float* combo_thr;        /* device [ncombo]: cumulative pick thresholds in (0, 1], non-decreasing, the last one 1 */
    const float* draws;            /* device [3, B]: u_full, u_partial, u_combo; NULL = evaluation form */
    const int* combo_idx;          /* device [B] or NULL: overrides the threshold pick (replay); -1 = no combination */
    float p_full, p_partial;
    int partial_on;
    unsigned int row_bits;         /* evaluation form: the bitmask of every row */
    int row_full;                  /* evaluation form: every row is full */
    int* counts;                   /* device int32[2 + ncomp] or NULL */
    int* row_combo;                /* device int32[B] or NULL: the combination each row took (-1: none or full) */
} lnx_meta_mask_args;
int lnx_meta_mask(const lnx_meta_mask_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * GPU-side image augmentations of the input pipeline: the tensor operations of the reference's
 * GPUAutoAugmentBatch (linnaeus/aug/gpu/autoaug.py:44-168) and GPURandomErasing (aug/gpu/random_erasing.py:24-94), on fp32
 * [B, C, H, W] batches, each followed by the clamp to [0, 1] the reference applies after every operation; plus the raw-image
 * conversion of h5data/prefetching_h5_dataset.py:214-220.  Which operation / rectangle is chosen stays on the host (the
 * Python classes of linnaeus_amd/aug.py draw exactly as the reference does).
 * -----------------------------------------------------------------------------------*/
enum {
    LNX_AUG_CLAMP = 0,
    LNX_AUG_POSTERIZE = 1,    /* floor(x 255 / p0) p0 / 255, p0 = 2^bits          autoaug.py:117-128 */
    LNX_AUG_SOLARIZE = 2,     /* x < p0 ? x : 1 - x                               :130-131 */
    LNX_AUG_SOLARIZE_ADD = 3, /* x < p1 ? clamp(x + p0) : x                       :133-138 */
    LNX_AUG_INVERT = 4,       /* 1 - x                                            :86 */
    LNX_AUG_BRIGHTNESS = 5,   /* p0 x (what :83-85 names: adjust_brightness)      */
    LNX_AUG_CONTRAST = 6      /* p0 x + (1 - p0) s[image] (adjust_contrast, s = mean grey level: lnx_aug_rowstat kind 1) */
};
/* in place; per_image_scalar: NULL or a device array with one float per image of `per_image` elements (a multiple of 4) */
int lnx_aug_pointwise(float* x, int64_t n, int64_t per_image, int op, float p0, float p1, const float* per_image_scalar, void* stream);
/* in place, three-channel images [B, 3, hw]: c <- clamp(f c + (1 - f) grey)  (Color / Desaturate, autoaug.py:114-115,153-154) */
int lnx_aug_saturation(float* x, int B, int64_t hw, float factor, void* stream);
/* kind 0: out[2r], out[2r+1] = min, max of row r of x [rows, cols]; kind 1: out[r] = mean grey level of RGB image r ([rows, 3, cols]) */
int lnx_aug_rowstat(const float* x, int rows, int64_t cols, int kind, float* out, void* stream);
/* in place: x[r, :] <- clamp((x - min_r) / (max_r - min_r + 1e-6)), minmax from lnx_aug_rowstat kind 0  (AutoContrast / Equalize, :143-151) */
int lnx_aug_rescale(float* x, int64_t rows, int64_t cols, const float* minmax, void* stream);
/* y[., h, w] = x[., round(sy), round(sx)], (sx, sy) = M (w - cx, h - cy) + (cx, cy), M = the host array m6 (2 x 3, output -> source),
 * nearest neighbour, zero outside: torchvision's affine / rotate on tensors with default interpolation and fill (:52-76) */
int lnx_aug_affine(const float* x, float* y, int planes, int H, int W, const float* m6, void* stream);
/* y = clamp(ratio x + (1 - ratio) (x * taps)), taps_dev = device [k, k]; mode 0 reflect padding (GaussianBlurRand, :156-165),
 * mode 1 borders keep x (Sharpness, :140-141) */
int lnx_aug_stencil(const float* x, float* y, int planes, int H, int W, const float* taps_dev, int k, int mode, float ratio, void* stream);
/* rects_dev = device int [n, 5] (image, y0, x0, h, w), values_dev = device float [n, C]: x[image, c, y0:y0+h, x0:x0+w] = value[c] */
int lnx_erase_rects(float* x, int B, int C, int H, int W, const int* rects_dev, const float* values_dev, int n_rects, void* stream);
/* raw image batch uint8 [B, H, W, C] -> fp32 [B, C, H, W] / 255 on the device (a quarter of the PCIe bytes of a float batch) */
int lnx_u8hwc_to_f32chw(const unsigned char* src, float* dst, int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------------------------------
 * Optimizer + step glue: multi-tensor AdamW with the global-norm clip folded in.
 * Replaces torch.optim.AdamW.step as configured by linnaeus/optimizers/build.py:307-686 (per-group lr / weight
 * decay) and the gradient-norm passes of train.py:282-308 (clip_grad_norm_ semantics:
 * coef = min(1, max_norm / (||g||_2 + 1e-6))).  `descs` is a DEVICE array, one entry per parameter tensor.
 *   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr/bias_c1 * m / (sqrt(v)/sqrt(bias_c2) + eps)
 * -----------------------------------------------------------------------------------*/
#define LNX_ADAMW_MAX_GROUPS 16
typedef struct lnx_adamw_desc {
    float* p;         /* parameter (fp32 master) */
    float* m;         /* exp_avg */
    float* v;         /* exp_avg_sq */
    const float* g;   /* gradient */
    int64_t n;        /* elements */
    int group;        /* index into lnx_adamw_hyper */
    int block_start;  /* first workgroup of this tensor: exclusive prefix sum of lnx_adamw_blocks(n) */
} lnx_adamw_desc;
typedef struct lnx_adamw_hyper {
    int ngroups;
    float lr[LNX_ADAMW_MAX_GROUPS], beta1[LNX_ADAMW_MAX_GROUPS], beta2[LNX_ADAMW_MAX_GROUPS], eps[LNX_ADAMW_MAX_GROUPS],
        weight_decay[LNX_ADAMW_MAX_GROUPS];
    float bias_c1[LNX_ADAMW_MAX_GROUPS], bias_c2[LNX_ADAMW_MAX_GROUPS]; /* 1 - beta^step of the step being taken */
    float omb1[LNX_ADAMW_MAX_GROUPS], omb2[LNX_ADAMW_MAX_GROUPS];       /* 1 - beta, rounded from double (1 - 0.999f loses 1e-5) */
} lnx_adamw_hyper;
int lnx_adamw_blocks(int64_t numel);
/* out[0] = sum over all tensors of g^2.  ws: total_blocks floats (one partial per workgroup, folded in a fixed order by a second
 * launch): the same gradients give the same bits on every data-parallel rank, so the clip coefficient -- and with it the
 * replicas' parameters -- cannot drift apart (clip_grad_norm_ of train.py:282-308 is deterministic in the same sense). */
int lnx_grad_sumsq(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, float* out, float* ws, void* stream);
/* sumsq == NULL or max_norm <= 0: no clipping */
int lnx_adamw_step(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_adamw_hyper* hyper, const float* sumsq, float max_norm,
                   void* stream);

/* AdEMAMix (linnaeus/optimizers/ademamix.py:119-175, built by optimizers/build.py:105-113 for OPTIMIZER.NAME = ademamix) over
 * the AdamW descriptor table, with the same clip: slow_dev is a DEVICE array parallel to descs_dev, slow_dev[i] = exp_avg_slow
 * of tensor i.  Per slot (one per (parameter group, step count) pair), with alpha_t / beta3_t the T_alpha_beta3 schedule of
 * ademamix.py:146-161 at that step (host, double, rounded once):
 *   p *= 1 - lr*wd;  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  s = beta3_t s + (1-beta3_t) g
 *   p -= lr/bias_c1 * (m + alpha_t s) / (sqrt(v)/sqrt(bias_c2) + eps)
 * The slow EMA is divided by bias_c1 too (as the reference does; the paper does not).  sumsq == NULL or max_norm <= 0: no clip. */
typedef struct lnx_ademamix_hyper {
    int ngroups;
    float lr[LNX_ADAMW_MAX_GROUPS], beta1[LNX_ADAMW_MAX_GROUPS], beta2[LNX_ADAMW_MAX_GROUPS], eps[LNX_ADAMW_MAX_GROUPS],
        weight_decay[LNX_ADAMW_MAX_GROUPS];
    float bias_c1[LNX_ADAMW_MAX_GROUPS], bias_c2[LNX_ADAMW_MAX_GROUPS]; /* 1 - beta^step of the step being taken */
    float omb1[LNX_ADAMW_MAX_GROUPS], omb2[LNX_ADAMW_MAX_GROUPS];       /* 1 - beta, rounded from double */
    float alpha_t[LNX_ADAMW_MAX_GROUPS], beta3_t[LNX_ADAMW_MAX_GROUPS], omb3[LNX_ADAMW_MAX_GROUPS]; /* scheduled; omb3 = 1 - beta3_t */
} lnx_ademamix_hyper;
int lnx_ademamix_step(const lnx_adamw_desc* descs_dev, float* const* slow_dev, int ndesc, int total_blocks, const lnx_ademamix_hyper* hyper,
                      const float* sumsq, float max_norm, void* stream);

/* torch.optim.SGD (built by optimizers/build.py for OPTIMIZER.NAME = sgd, always with nesterov) as one launch over the AdamW descriptor
 * table, with the same clip: desc.m is the momentum buffer (may be NULL only in slots with momentum 0), desc.v is not read.  Per slot:
 *   g *= coef;  g += weight_decay p;
 *   momentum != 0:  buf = first ? g : momentum buf + (1 - dampening) g;  g = nesterov ? g + momentum buf : buf
 *   p -= lr g
 * `first` marks the slot of parameters whose buffer does not exist yet (torch initialises it with the gradient): it is written, not read.
 * Refused on the host before any launch: NULL tables, ndesc <= 0, total_blocks <= 0, ngroups outside 1..LNX_ADAMW_MAX_GROUPS, a negative
 * lr, momentum or weight_decay, nesterov with momentum <= 0 or dampening != 0.  sumsq == NULL or max_norm <= 0: no clip.
 * 20 bytes per parameter, 12 without momentum. */
typedef struct lnx_sgd_hyper {
    int ngroups;
    float lr[LNX_ADAMW_MAX_GROUPS], momentum[LNX_ADAMW_MAX_GROUPS], dampening[LNX_ADAMW_MAX_GROUPS], weight_decay[LNX_ADAMW_MAX_GROUPS];
    int nesterov[LNX_ADAMW_MAX_GROUPS], first[LNX_ADAMW_MAX_GROUPS];
} lnx_sgd_hyper;
int lnx_sgd_step(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_sgd_hyper* hyper, const float* sumsq, float max_norm,
                 void* stream);
/* launches made by lnx_grad_sumsq (2), lnx_adamw_step, lnx_ademamix_step and lnx_sgd_step (1 each) and their _guarded forms since the
 * library was loaded (host-side counter, the twin of lnx_muon_launches) */
int64_t lnx_optim_launches(void);

/* Non-finite guard (lnx_version 117): the skipped step of torch.amp.GradScaler.step (train.py:279-312 of the reference steps through
 * scaler.step(optimizer)), decided once per step ON THE DEVICE.  All four fields are device pointers.
 *   lnx_grad_sumsq_guarded   the norm pass of lnx_grad_sumsq whose fold launch also decides: *flag = 1 when the sum of squares is not
 *                            finite (an inf or NaN gradient, or a finite one whose square overflows fp32, |g| >~ 1.8e19) or when
 *                            *found_inf != 0, else 0; then *skipped += *flag (one thread, ordinary stores).  `out` holds TWO floats:
 *                            out[0] the sum of squares as accumulated (of the scaled gradients when grad_scale is given), out[1] the
 *                            total norm of the unscaled gradients, sqrt(out[0]) * (1 / *grad_scale).
 *   lnx_*_step_guarded       every workgroup reads *flag first and returns when it is set: a skipped step writes nothing.  Otherwise,
 *                            with inv = 1 / *grad_scale (1 when grad_scale is NULL), the total norm is sqrt(*sumsq) * inv, the clip
 *                            coefficient min(1, max_norm / (norm + 1e-6)) and the gradient the update sees (g * inv) * coef, in that
 *                            order: a power-of-two scale gives the bits of the unscaled step.
 * found_inf and grad_scale may be NULL (no outside verdict, no scale); flag must be given; skipped is needed by the norm pass only.
 * guard == NULL: the entry point without the suffix, launch for launch and bit for bit. */
typedef struct lnx_step_guard {
    const float* found_inf;   /* GradScaler's verdict on the gradients, or NULL */
    const float* grad_scale;  /* the loss scale the gradients still carry, or NULL (already unscaled) */
    float* flag;              /* 1: this step is skipped; written by the norm pass, read by every step kernel */
    int64_t* skipped;         /* running count of skipped steps */
} lnx_step_guard;
int lnx_grad_sumsq_guarded(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, float* out, float* ws, const lnx_step_guard* guard, void* stream);
int lnx_adamw_step_guarded(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_adamw_hyper* hyper, const float* sumsq, float max_norm,
                           const lnx_step_guard* guard, void* stream);
int lnx_ademamix_step_guarded(const lnx_adamw_desc* descs_dev, float* const* slow_dev, int ndesc, int total_blocks, const lnx_ademamix_hyper* hyper,
                              const float* sumsq, float max_norm, const lnx_step_guard* guard, void* stream);
int lnx_sgd_step_guarded(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, const lnx_sgd_hyper* hyper, const float* sumsq, float max_norm,
                         const lnx_step_guard* guard, void* stream);

/* ------------------------------------------------------------------------------------
 * Muon (linnaeus/optimizers/muon.py:27-65, 126-190, chosen by OPTIMIZER.NAME = muon in optimizers/build.py:130-154): the whole step
 * for every 2-D / flattened 4-D parameter in 3 * max(ns_steps) + 3 launches, whatever the number of matrices.
 *   buf = lerp(buf, g, 1 - momentum);  u = nesterov ? lerp(g, buf, momentum) : buf          (muon.py:159-167, torch's lerp formulas)
 *   X = bf16(u), transposed when rows > cols;  X = bf16(X / (||X||_F + 1e-7))                (muon.py:45-52; norm and division in fp32)
 *   ns_steps times:  A = X X^T;  B = c A A + b A;  X = B X + a X                             (muon.py:55-58; a, b, c = 3.4445, -4.7750, 2.0315)
 *   p = p * decay - step * O,  decay = 1 - lr wd,  step = lr max(1, rows / cols)^(1/2)       (muon.py:156-157, 177-188)
 * Each product is a bf16 MFMA product with fp32 accumulation whose affine term is applied to the accumulator and rounded to bf16 once
 * (the reference rounds every product and every term).  g is not modified (the reference overwrites it with u, muon.py:167).
 *
 * Every matrix is held as X [m, n] with m = min(rows, cols), n = max(rows, cols), zero-padded to mp x np (multiples of
 * LNX_MUON_TILE); zero rows and columns stay zero through every product, so no kernel predicates an edge.  lnx_muon_layout places the
 * bf16 regions of every matrix in ONE workspace, which the caller allocates and zero-fills once:
 *   x_off          X [mp, np], updated in place by the third product (an element is read and written by the same lane only)
 *   xt_off[0..1]   X^T [np, mp], ping and pong: the third product reads one whole (its K runs along m) and writes the other
 *   a_off, b_off   A and B [mp, mp]
 * and lists the LNX_MUON_TILE x LNX_MUON_TILE output tiles of the three products in one table per stage (stage 0: A, 1: B, 2: X), the
 * tiles of matrix i at tile_start[s] .. + tile_count[s] of stage s.  A launch takes a PREFIX of a stage's table: order the matrices by
 * descending ns_steps and a matrix with fewer iterations drops out of the later launches.
 * No float atomics anywhere: sums of squares are per-workgroup partials folded in a fixed order (as lnx_grad_sumsq), the same inputs give the same bits.
 * -----------------------------------------------------------------------------------*/
#define LNX_MUON_TILE 32
#define LNX_MUON_ELEMS 4096 /* elements per workgroup of the momentum and apply launches */
typedef struct lnx_muon_mat {
    float* p;        /* parameter, fp32 [rows, cols] contiguous */
    float* buf;      /* momentum_buffer, fp32, same shape */
    const float* g;  /* gradient, or NULL: the parameter is skipped this step (muon.py:150-151) */
    int rows, cols;  /* logical shape; a 4-D parameter is [out, in * kh * kw] */
    int mp, np;      /* padded min(rows, cols), max(rows, cols) */
    int64_t x_off, xt_off[2], a_off, b_off; /* byte offsets in the workspace */
    int tile_start[3], tile_count[3];
    int block_start;                        /* first workgroup in the momentum / apply launches (= first sum-of-squares partial) */
    int ns_steps, nesterov;
    float momentum, omm;                    /* momentum and 1 - momentum, each rounded from double */
    float decay, step;                      /* 1 - lr wd and lr max(1, rows / cols)^(1/2): double on the host, rounded once */
} lnx_muon_mat;
typedef struct lnx_muon_tile {
    int mat, tr, tc, pad;                   /* output tile (tr, tc) of matrix mat */
} lnx_muon_tile;
typedef struct lnx_muon_info {
    int64_t workspace_bytes;
    int64_t ntiles[3];                      /* the three stage tables follow each other in `tiles` in this order */
    int total_blocks;
} lnx_muon_info;
/* Host side, no device work, no GPU needed.  shapes: n x [rows, cols].  Fills the geometry fields of mats[0..n) (pointers and
 * hyper-parameters are left alone), info, and -- when tiles != NULL -- the tile tables (tile_cap entries must hold them all). */
int lnx_muon_layout(const int* shapes, int n, lnx_muon_mat* mats, lnx_muon_tile* tiles, int64_t tile_cap, lnx_muon_info* info);
typedef struct lnx_muon_step_args {
    int n;
    const lnx_muon_mat* mats;        /* HOST copy: checked against lnx_muon_layout of its shapes before anything is launched */
    const lnx_muon_mat* mats_dev;    /* the same table on the device */
    const lnx_muon_tile* tiles_dev;  /* the tile tables lnx_muon_layout wrote, on the device */
    void* workspace;                 /* workspace_bytes, zero-filled once, 256-byte aligned */
    int64_t workspace_bytes;
    float* partials;                 /* total_blocks floats */
    /* appended (lnx_version 111): the global-norm clip of lnx_adamw_step.  sumsq is a DEVICE scalar, the sum of squares of every gradient
     * of the run (lnx_grad_sumsq); each gradient element is multiplied by min(1, max_norm / (sqrt(*sumsq) + 1e-6)) as it is read, before
     * the momentum lerp; g itself is not modified.  sumsq == NULL or max_norm <= 0 (a zero-filled tail): no clip, the step as before. */
    const float* sumsq;
    float max_norm;
    /* appended (lnx_version 117): the non-finite guard (lnx_step_guard above; a HOST pointer to the struct, its fields device pointers).
     * All 3 * ns + 3 launches read *guard->flag first and return when it is set: the momentum buffers, the parameters and the workspace
     * (whose zero padding is relied on for ever) stay as they were.  The momentum kernel reads the gradient as (g / *grad_scale) * coef.
     * NULL (a zero-filled tail): the step as before. */
    const lnx_step_guard* guard;
} lnx_muon_step_args;
int lnx_muon_step(const lnx_muon_step_args* args, void* stream);
/* launches made by lnx_muon_step, lnx_muon_orthogonalize and lnx_muon_apply_packed since the library was loaded (host-side counter, as
 * lnx_nt_kernel_launches) */
int64_t lnx_muon_launches(void);

/* Muon sharded over data-parallel ranks (lnx_version 118; the reference's DistributedMuon, muon.py:200-428): every rank holds the same
 * all-reduced gradients, orthogonalises only the matrices it OWNS, and the ranks all-gather the bf16 updates.  Each matrix gives the same
 * bits alone or in a set, so the sharded step gives the bits of lnx_muon_step.
 *   lnx_muon_partition      host only, no GPU, a pure function of its inputs: every rank computes the same table without communication.
 *                           Cost of matrix i: ns_steps (4 mp^2 np + 2 mp^3), the MFMA FLOPs of its three products with mp, np as
 *                           lnx_muon_layout pads them; mp np when ns_steps = 0.  Longest-processing-time greedy: the matrices by
 *                           (cost descending, index ascending), each to the least-loaded rank, the lowest rank on ties.  Inside a rank's
 *                           segment its matrices lie in table order, each at a multiple of LNX_MUON_SEG_ALIGN elements; *seg_elems is the
 *                           largest segment rounded up to that multiple (all_gather_into_tensor needs equal parts, so every segment is
 *                           padded to it).  owner and elem_off hold n entries, rank_cost holds world.
 *   lnx_muon_orthogonalize  the launches of lnx_muon_step over a table of the OWNED matrices (its layout, and so the workspace, is of
 *                           those alone) except the last: in place of the update, muon_pack_kernel writes each O as bf16 in logical
 *                           [rows, cols] row-major order (tall matrices are un-transposed here) at seg + out_off[i] elements.  p is not
 *                           touched; a matrix with g == NULL writes nothing; a step skipped by the guard writes nothing.
 *                           3 * max(ns_steps) + 3 launches.  out_off is given twice, as the table is: the host copy is checked (inside
 *                           seg_elems, multiples of LNX_MUON_SEG_ALIGN, pairwise disjoint), the device copy is what the kernel reads.
 *   lnx_muon_apply_packed   ONE launch over all matrices of the optimizer: p = p * decay - step * O, the expression of lnx_muon_step's last
 *                           launch, with O read from the gathered [world * seg_elems] bf16 buffer at `off` elements
 *                           (owner * seg_elems + elem_off).  An entry with off < 0 is skipped (a parameter without a gradient).  Obeys the
 *                           guard's flag (guard may be NULL).  block_start counts workgroups of LNX_MUON_ELEMS elements, skipped
 *                           entries included.  The host table is checked (offsets inside the gathered size, regions pairwise disjoint,
 *                           block_start) before the launch. */
#define LNX_MUON_SEG_ALIGN 128 /* elements: 256 bytes */
int lnx_muon_partition(const int* shapes, const int* ns_steps, int n, int world, int* owner, int64_t* elem_off, int64_t* seg_elems, int64_t* rank_cost);
int lnx_muon_orthogonalize(const lnx_muon_step_args* args, const int64_t* out_off_host, const int64_t* out_off_dev, void* seg, int64_t seg_elems, void* stream);
typedef struct lnx_muon_packed {
    float* p;        /* parameter, fp32 [numel] contiguous */
    int64_t off;     /* first element of its O in the gathered buffer, or < 0: skipped this step */
    int64_t numel;
    float decay, step;
    int block_start; /* first workgroup of the launch */
} lnx_muon_packed;
int lnx_muon_apply_packed(const lnx_muon_packed* table_host, const lnx_muon_packed* table_dev, int n, const void* gathered, int64_t seg_elems, int world,
                          const lnx_step_guard* guard, void* stream);

/* ------------------------------------------------------------------------------------
 * GradNorm task weighting (LOSS.GRAD_WEIGHTING.TASK.TYPE = gradnorm): loss/gradnorm.py GradNormModule.measure_and_update on the
 * device, behind one forward and one lnx_plan_backward_into per task (linnaeus_amd.loss.GradientWeighting).
 * lnx_gradnorm_sumsq: for task t < ntasks, sum of squares of the tensors of the AdamW-style descriptor table (only .g and .n are
 * read: the backbone slices of one gradient arena), with task t's gradients at .g + t * task_stride floats.  Same workgroup shape
 * and fixed-order two-pass fold as lnx_grad_sumsq (bit-identical to it per task).  Writes sumsq[t] (sumsq may be NULL) and
 * norm[t] = sqrt(sumsq[t]).  ws: ntasks * total_blocks floats.  ntasks <= LNX_MAX_TASKS.
 * -----------------------------------------------------------------------------------*/
int lnx_gradnorm_sumsq(const lnx_adamw_desc* descs_dev, int ndesc, int total_blocks, int ntasks, int64_t task_stride, float* sumsq, float* norm,
                       float* ws, void* stream);
/* lnx_gradnorm_update: one workgroup; every [T] array in sorted-task-key order (the order measure_and_update indexes task_weights in):
 *   loss_i = loss_sum_i / max(count_i, 1)
 *   first call with alpha > 0 (*initted == 0): initial_losses = init_loss (the all-reduced mean under data parallelism) or loss; *initted = 1
 *   g_avg = mean(norm);  alpha > 0: r_i = loss_i / max(L0_i, 1e-8), r_i *= T / max(sum r, 1e-8), target_i = g_avg r_i^alpha;
 *   alpha = 0: target_i = g_avg (r_i reported as 1)
 *   w_i *= norm_i / target_i unless target_i < 1e-8;  w *= T / max(sum w, 1e-8)
 * metrics (NULL or [1 + 5T]): g_avg, loss[T], norm[T], target[T], weight[T] (the new ones), ratio[T] (normalised). */
typedef struct lnx_gradnorm_args {
    int T;
    float alpha;
    const float* norm;      /* [T] backbone gradient norms */
    const float* loss_sum;  /* [T] sum of the per-sample losses over the valid rows */
    const float* count;     /* [T] valid rows */
    const float* init_loss; /* [T] or NULL */
    float* weights;         /* [T] task weights, updated in place */
    float* initial_losses;  /* [T] */
    int* initted;           /* device flag, 0 until initial_losses are set */
    float* metrics;
} lnx_gradnorm_args;
int lnx_gradnorm_update(const lnx_gradnorm_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * Validation metrics on the device: the per-batch bookkeeping of MetricsTracker._update_phase_batch
 * (linnaeus/utils/metrics/tracker.py:609-937) and of utils/metrics/chain_accuracy.py:143-166,299-344 as ONE launch that only ADDS to
 * two caller-owned, caller-zeroed device tables, int64 counts[] and double sums[]; nothing is read back, nothing is allocated.
 * Tasks come in ascending rank order (the tracker's `_L<n>` sort), n_tasks <= LNX_SOFTCE_MAX_TASKS.
 *   ordering   value descending, then index ascending; a NaN ranks above every number (torch.argmax / torch.topk).  A sample is
 *              top-1 (top-3) right when fewer than 1 (3) entries of its row come before its target's; with C < 3 correct3 = correct1
 *              (tracker.py:723-725).  A target outside [0, C) is never right.  Columns >= C of a padded row are never read.
 *   null split is_null[b] != 0, or target[b] == 0 where is_null is NULL; the chain figures always use target != 0.
 *   chain      every task right; partial_n: samples with some target != 0, partial_correct: those right on every task up to their
 *              highest non-null rank.
 *   subsets    per subset type s < 2 with subset_ids[s] != NULL: per task and bin, n and correct1; an id outside [0, n_bins[s])
 *              adds 1 to LNX_METRICS_SUBSET_OOR + s and nothing else.
 *   sums       per task with loss != NULL: loss[b] summed in double in a fixed order by one workgroup -- the same input gives the
 *              same bits on every run; LNX_METRICS_LOSS_N counts the samples summed.
 * counts layout (lnx_metrics_table_sizes gives the lengths):
 *   [0, LNX_METRICS_HEAD)                         the per-batch counters LNX_METRICS_CHAIN_N ...
 *   LNX_METRICS_TASK(t) + LNX_METRICS_N ...       the per-task counters
 *   LNX_METRICS_SUBSET(n_tasks, n_bins0, s) + 2 * (t * n_bins[s] + bin) + {0: n, 1: correct1}
 * sums layout: LNX_METRICS_SUM(t) + LNX_METRICS_SUM_LOSS ...
 * -----------------------------------------------------------------------------------*/
enum { LNX_METRICS_CHAIN_N = 0, LNX_METRICS_CHAIN_CORRECT, LNX_METRICS_PARTIAL_N, LNX_METRICS_PARTIAL_CORRECT, LNX_METRICS_SUBSET_OOR /* +s */,
       LNX_METRICS_HEAD = 8 };
enum { LNX_METRICS_N = 0, LNX_METRICS_CORRECT1, LNX_METRICS_CORRECT3, LNX_METRICS_NULL_N, LNX_METRICS_NULL_CORRECT1, LNX_METRICS_NONNULL_N,
       LNX_METRICS_NONNULL_CORRECT1, LNX_METRICS_LOSS_N, LNX_METRICS_TASK_STRIDE = 8 };
enum { LNX_METRICS_SUM_LOSS = 0, LNX_METRICS_SUM_NULL_LOSS, LNX_METRICS_SUM_NONNULL_LOSS, LNX_METRICS_SUM_STRIDE = 4 };
#define LNX_METRICS_TASK(t) (LNX_METRICS_HEAD + LNX_METRICS_TASK_STRIDE * (t))
#define LNX_METRICS_SUBSET(n_tasks, n_bins0, s) (LNX_METRICS_TASK(n_tasks) + ((s) ? 2 * (int64_t)(n_tasks) * (n_bins0) : 0))
#define LNX_METRICS_SUM(t) (LNX_METRICS_SUM_STRIDE * (t))
typedef struct lnx_metrics_task {
    const void* logits;           /* [B, ld] of the args' dtype */
    int64_t ld;                   /* >= C */
    const int64_t* target;        /* [B] class indices */
    const unsigned char* is_null; /* [B] or NULL (= target == 0) */
    const float* loss;            /* [B] per-sample losses or NULL */
    int C;
} lnx_metrics_task;
typedef struct lnx_metrics_args {
    int dtype; /* of every task's logits: 0 = fp32, 1 = bf16 */
    int B, n_tasks;
    lnx_metrics_task task[LNX_SOFTCE_MAX_TASKS];
    const int64_t* subset_ids[2]; /* [B] each, or NULL */
    int n_bins[2];                /* 0 where subset_ids[s] is NULL */
    int64_t* counts;
    double* sums;
} lnx_metrics_args;
int lnx_metrics_table_sizes(int n_tasks, int n_bins0, int n_bins1, int64_t* n_counts, int64_t* n_sums);
int lnx_metrics_update(const lnx_metrics_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * Predictions on the device: what LinnaeusInferenceHandler.predict (linnaeus/inference/handler.py:186-228) does per sample and task
 * with softmax / topk / .item(), followed by enforce_hierarchical_consistency (linnaeus/inference/postprocessing.py:14-171), as ONE
 * launch per batch that reads every logit once and writes the final lists.  Nothing is allocated, nothing is read back.
 * Tasks come FINEST FIRST (taxa_L10, taxa_L20, ...: DATA.TASK_KEYS_H5), n_tasks <= LNX_SOFTCE_MAX_TASKS.
 *   ordering   value descending, then index ascending; a NaN ranks above every number (the order of lnx_metrics_update).  It is taken
 *              on the logits as stored (bf16 -> float is exact), so the selected classes are exact.  Columns >= C are never read.
 *   probs      exp(x - max) / sum exp(x - max) in fp32 over the whole row whatever the storage type (the reference runs softmax in the
 *              logits' dtype under autocast); a row holding a NaN has NaN probabilities, a -inf entry has probability 0.
 *   raw        per sample b and task: the n = min(k_b, C) best entries, k_b = k_per_sample[b] clamped to [1, K], or K.
 *   chain      with consistency != 0, coarsest task first, keeping per sample the "consistent node" of the task above; for the coarsest
 *              task that is its raw top-1 class.  For a finer task t with raw top-1 class c:
 *                flag 1  the consistent node above is that task's null_index;
 *                flag 2  otherwise, parent[c] differs from the consistent node above (-1 always differs);
 *                flag 0  otherwise: kept, the consistent node becomes c.
 *              Flagged with null_index >= 0: the result becomes the single entry (null_index, 1.0f), count 1, and the consistent node
 *              null_index (postprocessing.py:124,141 write 1.0).  Flagged with null_index < 0: kept as it is, consistent node c
 *              (:128,145).  A coarsest task whose own top-1 is null keeps its raw entries (:153-154) and nullifies all below it.
 *   outputs    ids / probs [B, n_tasks, K], count / flags [B, n_tasks], all written in full: entries at or beyond count are
 *              (-1, 0.0f).  ids go through id_map where given (the nullified entry too).  consistency == 0: flags 0, nothing nullified.
 * -----------------------------------------------------------------------------------*/
#define LNX_PREDICT_MAX_K 16
typedef struct lnx_predict_task {
    const void* logits;    /* [B, ld] rows of the args' dtype, any row alignment */
    int64_t ld;            /* >= C */
    int C;
    const int32_t* parent; /* [C]: class index of this class's parent in the next coarser task, -1 = none; NULL for the coarsest task */
    int null_index;        /* the null class of this task (linnaeus: 0); < 0 = this task cannot be nullified */
    const int64_t* id_map; /* [C] class index -> the id written to ids[], or NULL (= the class index) */
} lnx_predict_task;
typedef struct lnx_predict_args {
    int dtype; /* of every task's logits: 0 = fp32, 1 = bf16 */
    int B, n_tasks;
    int K; /* 1 .. LNX_PREDICT_MAX_K */
    int consistency;
    const int32_t* k_per_sample; /* [B] or NULL (= K) */
    lnx_predict_task task[LNX_SOFTCE_MAX_TASKS];
    int64_t* ids;
    float* probs;
    int32_t* count;
    int32_t* flags;
} lnx_predict_args;
int lnx_predict(const lnx_predict_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * Image preprocessing on the device: what preprocess_image_batch / preprocess_single_image (linnaeus/inference/preprocessing.py:29-82)
 * do per image on one CPU thread -- TF.resize of a PIL image (Pillow's Image.resize on 8-bit RGB), TF.to_tensor, TF.normalize, then
 * torch.stack and a host-to-device copy -- for a whole batch of images of different sizes in at most two launches, in Pillow's own
 * integer arithmetic: the result equals the reference's bit for bit.
 *   bilinear / bicubic  two separable passes in 22-bit fixed point with a uint8 rounding between them.  One axis in -> out, in double:
 *                       scale = in / out, fs = max(scale, 1), support = S * fs (S = 1 bilinear, 2 bicubic), taps = 2 * ceil(support) + 1;
 *                       per output xx: center = (xx + 0.5) * scale, xmin = max((int)(center - support + 0.5), 0),
 *                       xmax = min((int)(center + support + 0.5), in), n = xmax - xmin; w[x] = f((x + xmin - center + 0.5) * (1 / fs)),
 *                       divided by their in-order sum when that is not 0; k[x] = (int)(w * 2^22 + 0.5) (w < 0: - 0.5).
 *                       A pass: out = clamp((2^21 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255), int32.  Horizontal first, only where the
 *                       width changes, into `scratch`; then vertical, only where the height changes.
 *   nearest             per axis a = in / out, xo = a * 0.5; per output in turn: index = min((int)xo, in - 1), xo += a.  (torchvision's
 *                       nearest_exact is the same for PIL inputs.)  One launch, no scratch.
 *   to_tensor/normalize out[i, c, y, x] = ((float)u8 / 255.0f - mean[c]) / std[c], both divisions correctly rounded.
 * lnx_resize_taps / lnx_resize_coeffs are host functions and need no GPU: the tables of one axis.  k is [out, taps] int32, zero beyond
 * n; bounds is [out, 2] int32 = (xmin, n).  Nearest: taps is 1, k is not written (may be NULL) and bounds is [out] source indices.
 *
 * The batch reaches the device as ONE buffer (`blob`, one host-to-device copy made by the caller): the descriptor table, the tables of
 * every distinct (in, out) pair and the packed [h, w, 3] uint8 sources, addressed by byte offsets.  lnx_preprocess_scratch_bytes fills
 * y0 / rows / htaps / vtaps / scratch of every descriptor from its h and w and returns the scratch the batch needs (< 0 on refusal);
 * lnx_preprocess checks every descriptor against that on the host copy before any launch, so the host copy and the one in the blob
 * must hold the same bytes.  Launches: bilinear / bicubic one per pass that any image needs (the vertical one also normalizes and
 * writes CHW, and runs as a copy for images whose height already fits); nearest one.  Nothing is allocated, nothing is read back.
 * -----------------------------------------------------------------------------------*/
#define LNX_RESIZE_NEAREST 0
#define LNX_RESIZE_BILINEAR 1
#define LNX_RESIZE_BICUBIC 2
#define LNX_PREPROCESS_MAX_SIDE 16384
int lnx_resize_taps(int in_size, int out_size, int filter); /* 0 on refusal */
int lnx_resize_coeffs(int in_size, int out_size, int filter, int32_t* k, int32_t* bounds);
typedef struct lnx_preprocess_image {
    int64_t src;     /* blob: [h, w, 3] uint8 */
    int64_t hk, hb;  /* blob: tables of the horizontal axis w -> W (multiples of 4; not read where w == W; nearest: hb alone) */
    int64_t vk, vb;  /* blob: tables of the vertical axis h -> H (not read where h == H) */
    int64_t scratch; /* scratch: the intermediate [rows, W, 3] uint8 of this image (set by lnx_preprocess_scratch_bytes) */
    int32_t h, w;    /* 1 .. LNX_PREPROCESS_MAX_SIDE */
    int32_t htaps, vtaps; /* lnx_resize_taps of the two axes, 0 where the pass does not run (set by lnx_preprocess_scratch_bytes) */
    int32_t y0, rows;     /* the source rows the vertical pass reads, [y0, y0 + rows): all the horizontal pass produces (set likewise) */
} lnx_preprocess_image;
typedef struct lnx_preprocess_args {
    int n, H, W;  /* images; output sides, 1 .. LNX_PREPROCESS_MAX_SIDE */
    int filter;   /* LNX_RESIZE_* */
    const lnx_preprocess_image* images; /* HOST copy of the descriptor table [n] */
    const void* blob;                   /* device, 16-byte aligned */
    int64_t blob_bytes;
    int64_t images_off; /* blob: the device copy of the descriptor table (multiple of 8) */
    void* scratch;      /* device; may be NULL when scratch_bytes is 0 */
    int64_t scratch_bytes;
    float mean[3], std[3]; /* std != 0 */
    float* out;            /* [n, 3, H, W] fp32 */
} lnx_preprocess_args;
int64_t lnx_preprocess_scratch_bytes(lnx_preprocess_image* images, int n, int H, int W, int filter);
int lnx_preprocess(const lnx_preprocess_args* args, void* stream);

/* ------------------------------------------------------------------------------------
 * The hierarchical loss of the train / validation step in a fixed number of launches: weighted_hierarchical_loss
 * (linnaeus/loss/hierarchical_loss.py:24-406) with apply_null_masking / apply_class_weighting / apply_loss_masking
 * (loss/masking.py:19-465, 469-518, 521-700) and GradientWeighting.forward (loss/gradient_weighting.py:301-358), for every task at once.
 * Replaces one lnx_softce launch per task and the chain of torch operations on [B] vectors behind it (and autograd's replay of it).
 * Per task t < n_tasks and row b < B, with the row arithmetic of lnx_softce (same NaN loss / zero gradient for a target outside [0, C)):
 *   class    target[b], or with soft_target the first maximum of soft_target[b, 0..C) (torch.argmax)
 *   raw      = crit_weight[class] * (lse * sum_c S[c] - sum_c S[c] x[c]),  S = soft[class, :] or the smoothed one-hot row; 0 where class == ignore_index
 *              (form LNX_CE_FORM_SOFT_ROW: S = soft_target[b, :] and sum_c soft_target[b, c] * crit_weight[c] in place of crit_weight[class];
 *               form LNX_CE_FORM_TAXONOMY: S = row `class` of the matrix that tax_anc / tax_val stand for, formed per column, soft == NULL)
 *   null     = target[b] == 0, or soft_target[b, 0] > 0.5
 *   keep     = !null || draws[t * B + b] < prob          (prob >= 1: everything is kept, prob <= 0: no null row; draws is read for 0 < prob < 1 only)
 *   masked   = keep ? raw : 0        (mask_mul != 0, the PHASE1_MASK_NULL_LOSS branch: raw * keep, so that a NaN survives the mask)
 *   cw       = class_weight[clamp(target, 0, n_cw - 1)] (1 where target >= n_cw), or with soft_target sum_c soft_target[b, c] * class_weight[c]
 *   nvalid   = count_b(masked != 0)   (before any class weight; mask_mul != 0: B, the reference divides by the batch size there)
 *   weighted = sum_b(masked * cw^p_w) / max(nvalid, 1e-6) * weights[t];   total = sum_t weighted   (fp32, in task order)
 *   dlogits[b, c] = go * scale[t] * coef[b] * (exp(x[c] - lse) * sum S - S[c]),  scale[t] = weights[t] / max(nvalid, 1e-6),
 *                   coef[b] = keep * cw^p_w * crit_weight[class] (0 for an ignored or out-of-range class); a row with coef == 0 is written as zeros
 * lnx_hier_loss_fwd: two launches -- one workgroup per (row, task), then ONE workgroup that folds every [B] sum in double, each thread a
 * fixed stride and a fixed LDS tree, so the same input gives the same bits.  lnx_hier_loss_bwd: one launch, reads ws / out of the forward
 * and the upstream gradient `go` from the device.  Nothing is allocated, nothing is read back.
 *   ws   [n_tasks][LNX_HL_WS_ROWS][B] floats: raw, lse, sum S, coef, masked * cw^p_cw, masked * cw^p_w, flags (bit 0 null, 1 keep, 2 masked != 0, the class from bit 3)
 *   out  [LNX_HL_OUT_FLOATS] floats: out[LNX_HL_OUT_x * LNX_SOFTCE_MAX_TASKS + t] for x in RAW_MEAN (mean raw), MASKED_MEAN (mean masked * cw^p_cw),
 *        WEIGHTED, SCALE; out[LNX_HL_OUT_TOTAL], out[LNX_HL_OUT_INCLUSION] (= 100 * null kept / max(null, 1) over all tasks)
 *   counts [LNX_HL_COUNTS] int64: nvalid[t] at t, rows with null at LNX_HL_NULL_TOTAL, null and kept at LNX_HL_NULL_INCLUDED
 * -----------------------------------------------------------------------------------*/
enum { LNX_HL_WS_RAW = 0, LNX_HL_WS_LSE, LNX_HL_WS_SS, LNX_HL_WS_COEF, LNX_HL_WS_MASKED_CW, LNX_HL_WS_MASKED_W, LNX_HL_WS_FLAGS, LNX_HL_WS_ROWS };
enum { LNX_HL_OUT_RAW_MEAN = 0, LNX_HL_OUT_MASKED_MEAN, LNX_HL_OUT_WEIGHTED, LNX_HL_OUT_SCALE, LNX_HL_OUT_TOTAL = 32, LNX_HL_OUT_INCLUSION = 33,
       LNX_HL_OUT_FLOATS = 40 };
enum { LNX_HL_NULL_TOTAL = 8, LNX_HL_NULL_INCLUDED = 9, LNX_HL_COUNTS = 10 };
typedef struct lnx_hier_loss_task {
    const void* logits;         /* [B, ld] of the args' dtype */
    int64_t ld;                 /* >= C */
    int C;
    const int64_t* target;      /* [B] class indices, or NULL with soft_target */
    const float* soft_target;   /* [B, ldt] mixup / cutmix targets, or NULL with target */
    int64_t ldt;                /* >= C */
    const float* soft;          /* [C, C] soft-label matrix, or NULL = one-hot with uniform smoothing */
    float smoothing;            /* soft == NULL only, in [0, 1) */
    const float* crit_weight;   /* [C] class weight of the criterion itself, or NULL */
    int64_t ignore_index;       /* < 0: none */
    const float* class_weight;  /* [n_cw] class weights of the task weighting, or NULL (then p_cw = p_w = 0) */
    int n_cw;                   /* >= C with soft_target */
    int p_cw, p_w;              /* 0..3, p_cw <= p_w: the power of cw in the logged masked loss and in the weighted loss (finding F13) */
    float* dlogits;             /* lnx_hier_loss_bwd: [B, ldd] fp32, columns >= C are not written; NULL = no gradient for this task */
    int64_t ldd;
    int form;                   /* LNX_CE_FORM_* of lnx_softce_args; 0 = the forms above.  LNX_CE_FORM_SOFT_ROW needs soft_target, which the
                                   backward reads again; null stays soft_target[b, 0] > 0.5 and the class in the flags the first maximum */
    /* appended (lnx_version 115): the tables of LNX_CE_FORM_TAXONOMY, as in lnx_softce_args; zero-filled with any other form.  With them
     * sizeof(lnx_hier_loss_task) is 152 and sizeof(lnx_hier_loss_args) 1280 bytes, passed by value to each kernel (limit: 4 KB) */
    const int32_t* tax_anc;
    const float* tax_val;
    int tax_depth;
} lnx_hier_loss_task;
typedef struct lnx_hier_loss_args {
    int dtype;            /* of every task's logits: 0 = fp32, 1 = bf16 */
    int B, n_tasks;       /* n_tasks <= LNX_SOFTCE_MAX_TASKS */
    float prob;           /* inclusion probability of null rows */
    int mask_mul;         /* != 0: masked = raw * keep and nvalid = B (PHASE1_MASK_NULL_LOSS in training) */
    const float* draws;   /* [n_tasks, B] uniform draws; required when 0 < prob < 1 */
    const float* weights; /* [n_tasks] task weights on the device */
    float* ws;
    float* out;
    int64_t* counts;
    lnx_hier_loss_task task[LNX_SOFTCE_MAX_TASKS];
} lnx_hier_loss_args;
int lnx_hier_loss_fwd(const lnx_hier_loss_args* args, void* stream);
int lnx_hier_loss_bwd(const lnx_hier_loss_args* args, const float* go_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Top-down refinement of the hierarchical heads (MODEL.CLASSIFICATION.HIERARCHICAL_REFINEMENT): what ConditionalClassifierHead.forward
 * (heads/conditional_classifier_head.py:191-224) and HierarchicalSoftmaxHead were written to do and never do (findings F3 / F4), in
 * ONE launch per direction for every level of every row.  Levels come FINEST FIRST, as in lnx_predict, n_tasks <= LNX_SOFTCE_MAX_TASKS.
 * Forward, from the coarsest level down; level t with parent level t + 1 and R = that level's finished `out` row AS STORED:
 *   prob   LNX_HIER_ROUTE_SOFT    softmax(R / temperature)
 *          LNX_HIER_ROUTE_GUMBEL  softmax((R + noise) / temperature), noise [B, C of level t + 1] fp32 supplied by the caller
 *          LNX_HIER_ROUTE_HARD    one-hot at the arg-max of R (torch.argmax: the lowest index on a tie, a NaN above every number)
 *   out[c] = base[c] + log(prob[parent[c]] + 1e-10),  prob = 0 where parent[c] < 0 (or beyond the parent level's C)
 *   The coarsest level and a level whose `parent` is NULL (no matrix for that pair) are passed through: out = base (not copied where
 *   out == base).  stats[b, t, 0..1] = the max and the sum of exponentials of level t's routing softmax (0, 0 for a pass-through).
 * Backward, from the finest level up: G_t = dout_t + (what level t - 1 sends up), dbase_t = G_t.  Level t - 1 sends to its parent t
 *   S[j] = sum of G_{t-1}[c] over the children c of j, dprob[j] = S[j] / (prob[j] + 1e-10),
 *   dR[j] = prob[j] * (dprob[j] - sum_k prob[k] dprob[k]) / temperature;  nothing for LNX_HIER_ROUTE_HARD or a NULL parent table.
 *   The children come from a CSR table: child_idx[child_start[j] .. child_start[j + 1]) in ascending class order, classes without a
 *   parent in no list.  The backward reads out, stats and noise of the forward, dout (NULL = zeros), and writes every dbase in full.
 * Storage of base / out / dout / dbase is the args' dtype, arithmetic fp32 (the segment sums accumulate in fp64); a level's row enters the next level as stored (rounded
 * to bf16 on bf16 tensors) in both directions.  Columns >= C are neither read nor written.  One workgroup per row walks the levels,
 * rows in strides (no class count has to fit on chip), fixed-order reductions, no atomics: bit-identical run to run.
 * Refused on the host before any launch: n_tasks outside 1..LNX_SOFTCE_MAX_TASKS, B <= 0, C <= 0, ld < C (backward: ldd < C), a NULL
 * stats / out / base (forward) / dbase (backward); and for every level that routes: temperature <= 0, an unknown mode, gumbel
 * without noise, and in the backward a parent table without child_start / child_idx.
 * -----------------------------------------------------------------------------------*/
enum { LNX_HIER_ROUTE_SOFT = 0, LNX_HIER_ROUTE_HARD = 1, LNX_HIER_ROUTE_GUMBEL = 2 };
typedef struct lnx_hier_refine_level {
    const void* base;           /* [B, ld] base logits (forward) */
    void* out;                  /* [B, ld] refined logits: written by the forward, read by the backward */
    const void* dout;           /* [B, ldd] gradient of out, or NULL = zeros (backward) */
    void* dbase;                /* [B, ldd] gradient of base (backward) */
    int64_t ld, ldd;            /* >= C */
    int C;
    int mode;                   /* LNX_HIER_ROUTE_*: how THIS level is routed from the level above */
    const int32_t* parent;      /* [C] class of the next coarser level, -1 = none (the convention of lnx_predict_task.parent); NULL = pass-through */
    const int32_t* child_start; /* [C of level t + 1, + 1] */
    const int32_t* child_idx;   /* [C] (as many entries as classes with a parent) */
    const float* noise;         /* [B, C of level t + 1] gumbel noise, LNX_HIER_ROUTE_GUMBEL only */
    float temperature;          /* > 0 */
} lnx_hier_refine_level;
typedef struct lnx_hier_refine_args {
    int dtype;    /* of base / out / dout / dbase of every level: 0 = fp32, 1 = bf16 */
    int B, n_tasks;
    float* stats; /* [B, n_tasks, 2] fp32 */
    lnx_hier_refine_level level[LNX_SOFTCE_MAX_TASKS];
} lnx_hier_refine_args;
int lnx_hier_refine_fwd(const lnx_hier_refine_args* args, void* stream);
int lnx_hier_refine_bwd(const lnx_hier_refine_args* args, void* stream);
/* launches made by lnx_hier_refine_fwd and lnx_hier_refine_bwd (1 each) since the library was loaded (host-side counter, the twin of
 * lnx_optim_launches) */
int64_t lnx_hier_refine_launches(void);

/* ------------------------------------------------------------------------------------
 * Abstention phase (the reference's phase 2: rl_train_abstention.py, rl_env/): batched rollout, rewards, advantages and the PPO loss
 * on [B, C] logits.  A decision at rank r depends on the image only, so a whole episode in either mode follows from ONE forward pass.
 * R ranks in DECISION order (r = 0 is decided first), 1 <= R <= LNX_SOFTCE_MAX_TASKS; logits fp32 or bf16, arithmetic fp32.
 * Per (b, r), from the row z = logits_r[b, 0..C):
 *   lse     = max + log(total),  total = the running sum of exp(z - max) below at its last class
 *   H       = lse - sum_c p[c] z[c]  (entropy; a term with p = 0 contributes 0, never NaN)
 *   greedy  = the arg-max, the lowest index on a tie
 *   action  greedy != 0: the arg-max.  Else the smallest j whose running sum of exp(z - max) in class order exceeds u[b, r] * total;
 *           if rounding leaves no such j, the arg-max.  u in [0, 1) is drawn by the caller.  The running sum is formed in a fixed
 *           order (256 contiguous chunks, an exclusive scan over the chunk sums, then class by class inside a chunk): the same
 *           input gives the same action on every run.
 *   logp    = z[action] - lse
 *   prediction None iff action == abstain_index (or the rank was not taken); ground truth None iff target[b] == null_index
 *   outcome = LNX_ABSTAIN_CORRECT (gt class, equal), CORRECT_ABSTAIN (None, None), MISCLASSIFIED (gt class, another class),
 *             UNNECESSARY_ABSTAIN (gt class, None), PREDICTED_AT_NULL (gt None, class): the argument order of SimpleAbstentionReward
 * Modes: LNX_ABSTAIN_MULTITASK decides every rank, one transition per sample (length = 1, logp_b = sum_r logp, H_b = sum_r H).
 *   LNX_ABSTAIN_SEQUENTIAL stops behind the first abstention: length L_b = its rank + 1, else R; ranks r >= L_b are not taken
 *   (taken = 0, action = abstain_index, logp = H = 0, prediction None, their rows are not read); transitions are (b, t), t < L_b, the
 *   reward falls on t = L_b - 1.
 * Reward of the episode over the counted ranks (LNX_ABSTAIN_RANKS_ALL: every rank, LNX_ABSTAIN_RANKS_FIRST: rank 0 only -- what the
 * reference's environment computes, finding F-a of INTEGRATION.md):
 *   LNX_ABSTAIN_REWARD_SIMPLE   sum of table[outcome] in rank order (fp32)
 *   LNX_ABSTAIN_REWARD_OUTCOME  the walk of EpisodeOutcomeReward: outcome_reward[0] if every rank up to and including the first
 *                               correct abstention is right (or all are, without one), else outcome_reward[1]
 * counts (NULL = none) is an int64 table of LNX_ABSTAIN_COUNTS entries this batch is ADDED to with integer atomics: per rank r at
 *   LNX_ABSTAIN_CNT_STRIDE * r the seven counters of the reference's evaluate_policy (every rank of every episode is one decision,
 *   an untaken one an abstention), then LNX_ABSTAIN_CNT_EPISODES, LNX_ABSTAIN_CNT_LENGTH_SUM and LNX_ABSTAIN_CNT_REWARD_FIX: the
 *   reward sum in units of 2^-LNX_ABSTAIN_REWARD_FIX_BITS (llrintf(reward * 2^20): exact for dyadic tables, order-free for any).
 * lnx_abstain_act: ONE launch, one workgroup per sample walking the ranks; three passes over a row (max; sum and sum e z in chunks;
 * the crossing inside one chunk).  No atomics on floats.
 * Refused on the host before any launch (all four entry points): R outside 1..8, B <= 0, C <= 0, ld < C, a NULL required pointer,
 * an abstain_index / null_index outside [0, C), an unknown dtype / mode / reward kind, a missing u without greedy.
 * -----------------------------------------------------------------------------------*/
enum { LNX_ABSTAIN_MULTITASK = 0, LNX_ABSTAIN_SEQUENTIAL = 1 };
enum { LNX_ABSTAIN_REWARD_SIMPLE = 0, LNX_ABSTAIN_REWARD_OUTCOME = 1 };
enum { LNX_ABSTAIN_RANKS_ALL = 0, LNX_ABSTAIN_RANKS_FIRST = 1 };
enum { LNX_ABSTAIN_CORRECT = 0, LNX_ABSTAIN_CORRECT_ABSTAIN, LNX_ABSTAIN_MISCLASSIFIED, LNX_ABSTAIN_UNNECESSARY_ABSTAIN, LNX_ABSTAIN_PREDICTED_AT_NULL,
       LNX_ABSTAIN_OUTCOMES };
enum { LNX_ABSTAIN_CNT_ABSTAINED = 0, LNX_ABSTAIN_CNT_TOTAL, LNX_ABSTAIN_CNT_CORRECT_ABSTAIN, LNX_ABSTAIN_CNT_UNNECESSARY_ABSTAIN, LNX_ABSTAIN_CNT_MISSED_ABSTAIN,
       LNX_ABSTAIN_CNT_CORRECT_CLASSIFY, LNX_ABSTAIN_CNT_MISCLASSIFY, LNX_ABSTAIN_CNT_STRIDE = 8, LNX_ABSTAIN_CNT_EPISODES = 64,
       LNX_ABSTAIN_CNT_LENGTH_SUM = 65, LNX_ABSTAIN_CNT_REWARD_FIX = 66, LNX_ABSTAIN_COUNTS = 72 };
#define LNX_ABSTAIN_REWARD_FIX_BITS 20
typedef struct lnx_abstain_rank {
    const void* logits;     /* [B, ld] of the args' dtype */
    int64_t ld;             /* >= C */
    int C;
    int abstain_index;      /* in [0, C): the class of this head that stands for "abstain" (lnx_abstain_act) */
    int null_index;         /* in [0, C): target == null_index is the ground truth None (lnx_abstain_act) */
    const int64_t* target;  /* [B] (lnx_abstain_act); a target outside [0, C) is a class no action equals */
    float* dlogits;         /* lnx_ppo_loss_bwd: [B, ldd] fp32; columns >= C and the rows of untaken ranks are not written */
    int64_t ldd;            /* >= C */
} lnx_abstain_rank;
typedef struct lnx_abstain_act_args {
    int dtype;                      /* of every rank's logits: 0 = fp32, 1 = bf16 */
    int B, R, mode, greedy, reward_kind, reward_ranks;
    float table[LNX_ABSTAIN_OUTCOMES]; /* LNX_ABSTAIN_REWARD_SIMPLE */
    float outcome_reward[2];        /* LNX_ABSTAIN_REWARD_OUTCOME: optimal, suboptimal */
    const float* u;                 /* [B, R] uniforms in [0, 1); may be NULL with greedy != 0 */
    int32_t* actions;               /* [B, R] */
    float* logp;                    /* [B, R] */
    float* entropy;                 /* [B, R] */
    uint8_t* taken;                 /* [B, R] */
    int32_t* length;                /* [B]: transitions of the episode (multitask: 1) */
    float* reward;                  /* [B] */
    int64_t* counts;                /* [LNX_ABSTAIN_COUNTS] or NULL */
    lnx_abstain_rank rank[LNX_SOFTCE_MAX_TASKS];
} lnx_abstain_act_args;
int lnx_abstain_act(const lnx_abstain_act_args* args, void* stream);

/* Advantages of whole episodes: the recursion of compute_gae_and_returns (rl_train_abstention.py:38-55) per episode, in fp32.  Every
 * episode of the rollout is complete, so next_non_terminal is 0 at its last step and the reference's last_value never enters.
 * Sequential: V_b at every step (the same image), reward[b] at t = L_b - 1 and 0 before; multitask: one step, slot [b, 0].
 *   adv[t] = delta_t + gamma * lambda * adv[t + 1],  delta_t = r_t + gamma * V_b * (t < L_b - 1) - V_b;   ret = adv + V_b
 * then adv = (adv - mean) / (std + 1e-8) over all N transitions of the rollout (population std).  mean and std are folded in double,
 * each thread a fixed stride and a fixed LDS tree: the same bits run to run.  Slots that are no transition are written as 0.
 * ONE launch of one workgroup.  n_trans[0] = N. */
typedef struct lnx_ppo_adv_args {
    int B, R, mode;
    float gamma, gae_lambda;
    const float* reward;    /* [B] */
    const float* value;     /* [B] */
    const int32_t* length;  /* [B], 1..R (multitask: ignored, 1) */
    float* adv;             /* [B, R] */
    float* ret;             /* [B, R] */
    int32_t* n_trans;       /* [1] */
} lnx_ppo_adv_args;
int lnx_ppo_advantages(const lnx_ppo_adv_args* args, void* stream);

/* The clipped-surrogate loss of ppo_update (rl_train_abstention.py:109-116) over the N transitions of a minibatch of B samples, each
 * decision evaluated at its own rank (finding F-d), with the row arithmetic of lnx_abstain_act (the same bits: a first epoch has
 * ratio = 1 exactly):
 *   ratio = exp(logp_new - logp_old);  policy = -mean(min(ratio A, clamp(ratio, 1 - eps, 1 + eps) A));  value = mean((V - ret)^2)
 *   entropy_loss = -mean(H);  total = policy + vf_coef * value + ent_coef * entropy_loss
 * multitask: logp_new - logp_old and H are summed over the ranks in rank order, A = adv[b, 0]; sequential: per taken (b, t).
 * lnx_ppo_loss_fwd: a launch of one workgroup per (sample, rank), then ONE workgroup that folds every sum in double in a fixed order.
 * lnx_ppo_loss_bwd: one launch; the gradients of torch autograd on the expression above (d/dratio = A where ratio A <= the clipped
 * term, else 0), times the device scalar go_dev[0]: rank[r].dlogits (NULL = none for that rank) and dvalue [B] (NULL = none), which
 * in sequential mode sums the L_b steps of sample b.
 *   ws   [R][LNX_PPO_WS_ROWS][B] floats (lse, H, logp_new, the transition's d total / d logp_new times N)
 *   out  [LNX_PPO_OUT_FLOATS] floats at LNX_PPO_OUT_* */
enum { LNX_PPO_WS_LSE = 0, LNX_PPO_WS_H, LNX_PPO_WS_LOGP, LNX_PPO_WS_COEF, LNX_PPO_WS_ROWS };
enum { LNX_PPO_OUT_POLICY = 0, LNX_PPO_OUT_VALUE, LNX_PPO_OUT_ENTROPY, LNX_PPO_OUT_TOTAL, LNX_PPO_OUT_N, LNX_PPO_OUT_RATIO_MEAN, LNX_PPO_OUT_CLIP_FRAC,
       LNX_PPO_OUT_FLOATS = 8 };
typedef struct lnx_ppo_loss_args {
    int dtype, B, R, mode;
    float clip_eps, vf_coef, ent_coef;
    const int32_t* actions;  /* [B, R] */
    const uint8_t* taken;    /* [B, R] */
    const float* logp_old;   /* [B, R] */
    const float* adv;        /* [B, R] */
    const float* ret;        /* [B, R] */
    const float* value;      /* [B] */
    float* ws;
    float* out;
    float* dvalue;           /* lnx_ppo_loss_bwd: [B] or NULL */
    lnx_abstain_rank rank[LNX_SOFTCE_MAX_TASKS];
} lnx_ppo_loss_args;
int lnx_ppo_loss_fwd(const lnx_ppo_loss_args* args, void* stream);
int lnx_ppo_loss_bwd(const lnx_ppo_loss_args* args, const float* go_dev, void* stream);
/* kernel launches made by the four entry points above since the library was loaded (host-side counter): 1 for lnx_abstain_act, 1 for
 * lnx_ppo_advantages, 2 for lnx_ppo_loss_fwd, 1 for lnx_ppo_loss_bwd */
int64_t lnx_abstain_launches(void);

/* ------------------------------------------------------------------------------------
 * Fused ConvNeXt MLP branch (bf16 storage, C in {32,64,96,128,192}):
 *   out = x + rowscale * gamma * (GELU(ln . W1^T + b1) . W2^T + b2)
 * = pwconv1 -> GELU -> pwconv2 -> LayerScale -> DropPath -> residual (blocks/convnext.py:79-86)
 * with the 4C hidden activation kept on chip; the backward recomputes it per tile.
 * -----------------------------------------------------------------------------------*/
int lnx_convmlp_supported(int dtype, int C);
typedef struct lnx_convmlp_args {
    int dtype, M, C;
    const void* ln;        /* [M, C] bf16 (block LayerNorm output) */
    const void* w1;        /* [4C, C] bf16 pwconv1.weight */
    const float* b1;       /* [4C] */
    const void* w2;        /* [C, 4C] bf16 pwconv2.weight */
    const float* b2;       /* [C] */
    const float* gamma;    /* [C] */
    const float* rowscale; /* per-sample DropPath multiplier or NULL */
    int rows_per_sample;
    const float* x;        /* [M, C] fp32 residual input */
    float* out;            /* [M, C] fp32 */
    void* z;               /* optional [M, C] bf16: pwconv2 output before gamma (for the gamma gradient) */
    /* Fused block LayerNorm (blocks/convnext.py:77,84 `x = self.norm(x)`, eps 1e-6; round 3): with `y` set the kernel reads the
     * LayerNorm INPUT (the depthwise conv output) and normalises it in registers -- `ln` must then be NULL -- and writes what the
     * backward needs: the normalised rows (operand of the pwconv1 weight gradient) and the row statistics. */
    const void* y;         /* [M, C] bf16, or NULL: `ln` is given */
    const float* ln_w;     /* [C] */
    const float* ln_b;     /* [C] */
    float ln_eps;
    void* ln_out;          /* optional out [M, C] bf16 */
    float* mean;           /* optional out [M] (with rstd) */
    float* rstd;
    /* DropPath compaction (lnx_drop_partition; both NULL = every row in natural order).  The kernel walks COMPACT rows: row m' < *m_dev
     * is sample perm[m' / rows_per_sample], pixel m' % rows_per_sample (rows_per_sample | M).  x, y and out keep natural sample order
     * and are addressed through perm; ln (in or out), mean and rstd hold compact rows, rows >= *m_dev are neither read nor written.
     * Kept rows get the bits of the full-row call; the rows of out that belong to dropped samples are copies of their rows of x (by
     * the kernel itself: no launch is added).  z must be NULL. */
    const int* perm;       /* [M / rows_per_sample] device: kept samples first */
    const int* m_dev;      /* device int: kept samples x rows_per_sample */
} lnx_convmlp_args;
int lnx_convmlp_fwd(const lnx_convmlp_args* args, void* stream);

typedef struct lnx_convmlp_bwd_args {
    int dtype, M, C;
    const float* g;        /* [M, C] fp32 gradient of the block output */
    const void* ln;        /* [M, C] bf16 */
    const void* z;         /* [M, C] bf16 saved by the forward, or NULL (round 4): dgamma is then NOT produced here -- see
                              lnx_layerscale_apply_wgrad */
    const void* w1;        /* [4C, C] bf16 */
    const float* b1;
    const void* w2t;       /* [4C, C] bf16 = pwconv2.weight^T */
    const void* w1t;       /* [C, 4C] bf16 = pwconv1.weight^T */
    const float* gamma;
    const float* rowscale;
    int rows_per_sample;
    void* act;             /* out [M, 4C] bf16  GELU(h)   (operand of the pwconv2 weight gradient), or NULL with dh NULL: */
    void* dh;              /* out [M, 4C] bf16  dL/dh     (operand of the pwconv1 weight gradient)   not materialised  */
    void* dz;              /* out [M, C]  bf16  rowscale*gamma*g */
    void* dln;             /* out [M, C]  bf16  gradient wrt the LayerNorm output */
    float* dgamma;         /* [C] += : LDS float atomics across the waves and one global float atomic per workgroup, or (deterministic mode)
                              a [C] row per WAVE in ws behind the LayerNorm rows, folded in row order and added once -- ws is then
                              required with z as well */
    /* Fused LayerNorm backward (round 3): with `y` set, `dln` receives the gradient wrt the LayerNorm INPUT y instead (what
     * lnx_layernorm_bwd would make of dln, y, mean, rstd), and d_ln_w / d_ln_b += the LayerNorm weight / bias gradient. */
    const void* y;         /* [M, C] bf16, or NULL */
    const float* ln_w;     /* [C] */
    const float* mean;     /* [M] saved by the forward */
    const float* rstd;
    float* d_ln_w;         /* [C] += */
    float* d_ln_b;         /* [C] += */
    float* ws;             /* scratch for the per-workgroup column sums: lnx_convmlp_bwd_ws_floats(C, M) floats (2 C per workgroup */
    int64_t ws_floats;     /* of the launch this library would make for (C, M)); too small = error                              */
    int dz_plain;          /* round 4.  != 0: the `dz` written to memory is rowscale * g, WITHOUT the LayerScale factor gamma (inside the
                              kernel the data gradient keeps it): the dY operand of a pwconv2 weight-gradient product whose result
                              lnx_layerscale_apply_wgrad multiplies by gamma afterwards (and reads the LayerScale gradient from) */
    int ln_defer;          /* round 5.  != 0 (fused LayerNorm form): the fold of the workgroups' column sums into d_ln_w / d_ln_b is postponed to
                              lnx_layernorm_bwd_flush() together with the postponed LayerNorm backward calls; `ws` must stay untouched until then */
    /* DropPath compaction, as in lnx_convmlp_args (both NULL = every row).  g, y and dln keep natural sample order and are addressed
     * through perm; ln, mean, rstd, act, dh and dz hold compact rows, rows >= *m_dev are neither read nor written and stay out of every
     * column sum (dgamma, d_ln_w, d_ln_b).  The rows of dln that belong to dropped samples are not written (the depthwise gradients take
     * the same list and do not read them); g is only read.  The weight-gradient products over act / dh / dz / ln take the same m_dev.
     * z must be NULL. */
    const int* perm;
    const int* m_dev;
} lnx_convmlp_bwd_args;
int lnx_convmlp_bwd(const lnx_convmlp_bwd_args* args, void* stream);
/* floats of `ws` the fused-LayerNorm backward needs for (C, M), from the same grid choice the launcher makes (0: unsupported C).
 * Deterministic mode: the larger need of its routes -- a [2C] LayerNorm row and a [C] dgamma row per wave (8 a workgroup; 4 at
 * C >= 128 with LNX_CM_NW=4) instead of [2C] per workgroup; the rows are folded in row order by the shared second stage.  A ws that
 * is too small for the mode the call runs in is refused by name. */
int64_t lnx_convmlp_bwd_ws_floats(int C, int M);

/* (round 2 had lnx_convmlp_wgrad here: both weight gradients from ln / dz with the hidden recomputed on chip, so that act / dH
 * never reached HBM.  Correct, but slower end to end on MI355X -- 302 + 207 us per block at C = 96 against 317 us for the two
 * weight-gradient GEMMs it replaced, because a single launch cannot hold the 288 KB of dW1 + dW2 accumulators and each of the two
 * launches re-evaluates the GELU -- and removed in round 3; DESIGN.md records the numbers.) */

/* ------------------------------------------------------------------------------------
 * Whole-model plan: mFormerV1 forward and backward as one native call each.
 * Replaces mFormerV1.forward_features/forward (models/mFormerV1.py:407-541) and its
 * autograd backward.  The plan owns no memory: the caller passes one workspace of
 * lnx_plan_workspace_bytes() bytes (activations saved for backward, the T-typed operand
 * arena, scratch) and binds parameter / gradient pointers in the plan's parameter order
 * (= the reference's state_dict order, see lnx_plan_param_name).
 * -----------------------------------------------------------------------------------*/
#define LNX_MAX_META 8
#define LNX_MAX_TASKS 16
typedef struct lnx_mformer_cfg {
    int dtype;                 /* LNX_F32 (strict parity) or LNX_BF16 */
    int batch, img_h, img_w, in_chans;
    int dims[4];               /* CONVNEXT_STAGES.DIMS (dims[2:] are the RoPE dims) */
    int conv_depths[2];        /* CONVNEXT_STAGES.DEPTHS[0:2] */
    int rope_depths[2];
    int rope_heads[2];         /* dims[2+s] / rope_heads[s] = head_dim: 32, 64 or 128 */
    int mlp_hidden[2];         /* int(dim * MLP_RATIO) */
    int n_meta;                /* enabled metadata components, 0 = metadata inactive */
    int meta_dims[LNX_MAX_META];
    int only_last_cls;
    int n_tasks;
    int task_classes[LNX_MAX_TASKS];
    int inference;             /* 1: forward-only plan (model.eval() under no_grad, validation.py:199): no backward scratch,
                                  blocks share their activation buffers; lnx_plan_backward fails on it */
    int recompute;             /* 1: activation recompute (gradient checkpointing, blocks/convnext.py:89-100,
                                  rope_2d_mhsa.py:617-641): only each block's INPUT is kept; the blocks of a stage share one
                                  set of activation buffers and lnx_plan_backward re-runs a block's forward right before its
                                  backward.  Same results bit for bit (the recompute is deterministic and reuses the DropPath
                                  draw of the forward); workspace no longer grows with the depth. */
    int fp8;                   /* 1 (with dtype = LNX_BF16): the forward products of the RoPE blocks' qkv / fc1 / fc2 Linear layers run
                                  on the block-scaled fp8 matrix cores (MXFP8: lnx_quantize_mxfp8 + lnx_gemm_nt_mxfp8) -- BASELINE
                                  config 5's "fp8 MFMA path".  Weights are re-quantised from the fp32 masters every forward,
                                  activations as they are produced; everything saved for the backward stays bf16.  In the backward
                                  the proj / fc2 / fc1 data-gradient products run in MXFP8 as well (gradients quantised per
                                  32-element block, dY as the MXFP8 copy the LayerNorm backward writes beside its bf16 output --
                                  measured: +1 % speed at xl for a quarter more gradient error); environment LNX_FP8_DGRAD=0,
                                  read at plan creation, keeps them bf16.  Needs RoPE dims and MLP widths that are multiples
                                  of 128. */
    int rope_mode;             /* LNX_ROPE_COS (0, the reference as it runs) or LNX_ROPE_ROTATE (MODEL.ROPE_STAGES.ROPE_ROTATE): every RoPE
                                  block's attention rotates q and k (see lnx_attn_args.rope_mode) in the forward, the backward and a
                                  recompute plan's re-forward; the one-launch table fill writes cos and sin tables (the sin table takes
                                  the place of the d-cos table in the workspace).  Parameters, their order and shapes do not change. */
} lnx_mformer_cfg;

typedef struct lnx_plan lnx_plan;
int lnx_plan_create(const lnx_mformer_cfg* cfg, lnx_plan** out);
void lnx_plan_destroy(lnx_plan* p);
int64_t lnx_plan_workspace_bytes(const lnx_plan* p);
int lnx_plan_num_params(const lnx_plan* p);
/* "stem.0.weight", "stages.2.0.attn.freqs", ...; heads are "head.<task index>.weight|bias" */
const char* lnx_plan_param_name(const lnx_plan* p, int i);
int64_t lnx_plan_param_numel(const lnx_plan* p, int i);
int lnx_plan_num_drop_calls(const lnx_plan* p);
/* logits are written as one fp32 buffer: task t occupies [batch, ld_t] at element offset off_t */
int64_t lnx_plan_logits_numel(const lnx_plan* p);
int64_t lnx_plan_logits_offset(const lnx_plan* p, int task);
int lnx_plan_logits_ld(const lnx_plan* p, int task);
/* Bind device pointers: params[i] / grads[i] fp32 in plan order (grads may be NULL for an
 * inference-only plan), workspace of lnx_plan_workspace_bytes().  Synchronises the device once. */
int lnx_plan_bind(lnx_plan* p, const float* const* params, float* const* grads, void* workspace);
/* x [B,Cin,H,W] fp32 NCHW, meta [B, sum(meta_dims)] fp32 or NULL, drop_scales [n_drop_calls, B]
 * fp32 per-sample DropPath multipliers (NULL = eval / no DropPath), drop_mask[i] != 0 selects
 * which calls use their row.  Outputs: feats [B, dims[3]] fp32, logits (layout above). */
int lnx_plan_forward(lnx_plan* p, const float* x, const float* meta, const float* drop_scales, const unsigned char* drop_mask,
                     float* feats, float* logits, void* stream);
/* Metadata variants from one trunk pass (lnx_version 120).
 * Re-run an inference plan from the token boundary with other metadata: the metadata heads, both RoPE stages,
 * norm_1 / cl_1_fc / downsample 2 (model index; plan.cpp calls it downsample 3), the tail and the heads.
 * Needs a completed lnx_plan_forward on this plan whose stem / ConvNeXt / downsample-1 results are still in place.
 * feats / logits as in lnx_plan_forward; they receive what lnx_plan_forward(p, x, meta, NULL, NULL, ...) with that forward's x would
 * write, bit for bit (the same kernels on the same operands: the metadata enters only as the extra token rows of the two RoPE stages).
 * The metadata heads run on `stream` itself (no side stream, no events).  No workspace beyond the plan's, no copy: the stage-3 token
 * buffer is read-only to the RoPE blocks, so the forward's patch rows are still there.
 * Rules for the caller:
 *  - the tail must be ordered after the forward on the same stream (or by the caller's own events); so must successive tails, and
 *    whoever reads feats / logits of one call before the next call on this plan overwrites the workspace (not those buffers);
 *  - the tail sees the weights as of that forward (the operand arena is refreshed by lnx_plan_forward only) and follows that forward's
 *    CLS-only decision (lnx_set_last_cls);
 *  - any later lnx_plan_forward starts a new trunk; lnx_plan_bind and any failed lnx_plan_forward / lnx_plan_forward_tail discard it.
 * Refused before any launch (nonzero, lnx_last_error): a NULL or unbound plan, a training or recompute plan, a plan without
 * metadata components, NULL meta, NULL logits with tasks configured, no valid trunk.
 * lnx_plan_trunk_valid: 1 if lnx_plan_forward_tail may be called, else 0. */
int lnx_plan_forward_tail(lnx_plan* p, const float* meta, float* feats, float* logits, void* stream);
int lnx_plan_trunk_valid(const lnx_plan* p);   /* 1: lnx_plan_forward_tail may be called */
/* Training-time dropout of the RoPE blocks (MODEL.DROP_RATE): keep masks for the next forward and its backward, one byte per
 * element, per RoPE block (stage 3 blocks first) [proj output M x C][MLP hidden M x hidden][fc2 output M x C] -- the caller
 * draws them (Bernoulli(1 - drop_rate)) and keeps the buffer alive until the backward has run.  masks = NULL or
 * drop_rate = 0 switches dropout off.  Not available on fp8 or inference plans. */
int64_t lnx_plan_dropout_bytes(const lnx_plan* p);
int lnx_plan_set_dropout(lnx_plan* p, const unsigned char* masks, float drop_rate);
/* The same for MODEL.ATTN_DROP_RATE (dropout on the attention probabilities, rope_2d_mhsa.py:497): per RoPE block a keep
 * mask [B, heads, N, Np] (Np = N rounded up to a multiple of 64), see lnx_attn_args.drop_mask. */
int64_t lnx_plan_attn_dropout_bytes(const lnx_plan* p);
int lnx_plan_set_attn_dropout(lnx_plan* p, const unsigned char* masks, float drop_rate);
/* Backward of the last forward.  dlogits has the logits layout; dfeats [B, dims[3]] is an
 * optional extra gradient on feats (NULL).  Parameter gradients are ACCUMULATED into the bound
 * grads.  segment: -1 = everything, or 0..3 = {tail + RoPE stage 4, RoPE stage 3, ConvNeXt
 * stage 2, ConvNeXt stage 1 + stem}, to be called in that order (lets the caller start the
 * gradient all-reduce of a finished segment while the next one runs). */
int lnx_plan_backward(lnx_plan* p, const float* dlogits, const float* dfeats, int segment, void* stream);
/* lnx_plan_backward(segment = -1) with the parameter gradients ACCUMULATED into grads[lnx_plan_num_params] (fp32, 4-byte aligned)
 * instead of the bound ones, which stay untouched and are bound again when the call returns, whatever it returns.  No rebind:
 * the forward stays valid, and any number of these (and lnx_plan_backward) may follow one forward, each giving what a fresh
 * forward + backward would (recompute plans re-run every block, the last ones included).  GradNorm runs one forward and one
 * of these per task, seeded by that task's dlogits alone, into scratch gradient arenas.  It never writes input gradients
 * (lnx_plan_bind_input_grads): dx / dmeta stay as they are. */
int lnx_plan_backward_into(lnx_plan* p, const float* dlogits, const float* dfeats, float* const* grads, void* stream);
/* Live per-kernel-class timing with HIP events on the launch stream (used by bench.py for the
 * roofline line; adds event records around the timed launches, so never leave it on in a timed
 * region).  Classes: 0 gemm_nt, 1 gemm_tn, 2 attention fwd, 3 attention bwd (both kernels),
 * 4 depthwise conv fwd / data-grad, 5 depthwise conv weight-grad, 6 fused conv-MLP forward,
 * 7 fused conv-MLP backward (data side), 8 fused conv-MLP weight gradients.  work = FLOPs for 0-3 and 6-8,
 * algorithmic HBM bytes for 4-5. */
#define LNX_PROFILE_CLASSES 8
int lnx_plan_profile_begin(lnx_plan* p);
int lnx_plan_profile_end(lnx_plan* p, double* ms, double* work, int* launches);
/* Round 4.  lnx_plan_profile_end_ex: as lnx_plan_profile_end with LNX_PROFILE_CLASSES_EX entries per array and, per class, the
 * ALGORITHMIC HBM bytes of its launches (every operand read once, every output written once; GEMM classes 0 / 1 only) -- what
 * bench.py's roofline object prices the achieved TB/s and the FLOP/byte of the dominant class with.
 * lnx_plan_profile_begin_spans: block-level timing instead of per-launch timing -- ONE event pair around each whole block on
 * the main stream, forward and backward (incl. a recompute plan's re-forward): class 8 = RoPE2DMHSABlock (rope_2d_mhsa.py:584-645:
 * both LayerNorms, qkv, attention, proj, Mlp, their weight gradients and reduces), work = the block's FLOPs (forward 1x +
 * backward 2x of its GEMM and attention products: BASELINE.md's 15.94 GFLOP/img for mFormerV1_sm); class 9 = ConvNeXtBlock
 * (convnext.py:73-87).  No events sit between the kernels of a block, so the span is what the block costs in the timed step. */
#define LNX_PROFILE_CLASSES_EX 10
int lnx_plan_profile_begin_spans(lnx_plan* p);
int lnx_plan_profile_end_ex(lnx_plan* p, double* ms, double* work, double* bytes, int* launches);
/* Round 4: the backward's weight-gradient stream.  By default a plan runs the RoPE blocks' weight-gradient products (+ their batched
 * split-K reduce) and the fused ConvNeXt blocks' pointwise weight gradients (+ the LayerScale step) on a HIP stream of its own, forked
 * behind the kernel that wrote each product's dY and joined before that buffer's next writer and at the end of every block -- the
 * same kernels, the same sums in the same order (bit-equal gradients), ramps and tails of one chain under the body of the other.
 * lnx_plan_set_wgrad_stream(p, 0) puts everything back on the launch stream (what bench.py's per-kernel timing pass does, so that a
 * kernel's duration is its own); returns the previous setting (0 / 1), negative on error.  LNX_WGRAD_STREAM=0 never creates the stream. */
int lnx_plan_set_wgrad_stream(lnx_plan* p, int on);
/* Round 5: which stream the metadata heads (forward chain, backward chain + weight gradients) run on beside the launch stream:
 * 0 = the launch stream itself, 1 = a side stream of their own (default; LNX_NO_SIDE_STREAM never creates it), 2 = the weight-gradient
 * stream (one HIP stream fewer: a data-parallel step then uses launch + weight-gradient streams + the collective library's own --
 * within the four hardware queues of the device; only with the one-launch chain, otherwise as 1).  Forks and joins are events either
 * way: same values, same summation orders.  Returns the previous mode, negative on error.  LNX_META_STREAM=0/1/2 sets the default. */
int lnx_plan_set_meta_stream(lnx_plan* p, int mode);
/* indices of the parameters whose gradient is final after `segment`; returns their count.  The metadata heads' backward
 * runs on the plan's side stream and is joined one segment after the one that forks it, so the stage-4 heads report
 * segment 1 and the stage-3 heads segment 2 (a caller that stops early must run the following segment, or -1, to join). */
int lnx_plan_segment_params(const lnx_plan* p, int segment, int* idx_out, int max_out);

/* Fine-tuning: a frozen prefix (lnx_version 112).  The reference freezes parameters by requires_grad (its parameter filters,
 * rl_train_abstention.py:368-403); autograd then neither saves activations for, nor differentiates, what lies before the first
 * trainable parameter.  A plan does the same at the granularity of UNITS, a fixed list in forward order:
 *     stem | stages.0.<i> | downsample_layers.0 | stages.1.<i> | downsample_layers.1 | tokens_1 | stages.2.<i> | mid | tokens_2 |
 *     stages.3.<i> | tail | heads
 * tokens_k = cls_token_k and every metadata head of RoPE stage k; mid = norm_1, cl_1_fc, downsample_layers.2; tail = norm_2, aggregate,
 * final_norm; heads = every head.<t>.  Every plan parameter belongs to exactly one unit.
 *   lnx_plan_num_units / lnx_plan_unit_name(u) / lnx_plan_param_unit(i)   the list, and the unit of parameter i
 *   lnx_plan_set_trainable(mask)   mask[i] != 0: parameter i (plan order, lnx_plan_num_params bytes) trains.  The CUT is the first unit
 *       that holds a trainable parameter.  Legal only between lnx_plan_create and lnx_plan_bind (it changes lnx_plan_workspace_bytes);
 *       refused by name on an inference plan, after the bind, with a NULL mask and with an all-zero mask (that is an inference plan).
 *       Not calling it, or a mask whose cut is the stem (all ones), is the plan as created: same workspace bytes, same launches, same bits.
 *   lnx_plan_first_trained_unit    the cut (0 when nothing is frozen)
 *   lnx_plan_last_backward_units   units the last lnx_plan_backward (segment -1, or the segments 0..3 summed) / lnx_plan_backward_into ran
 * With a cut at unit u:
 *   forward   every unit runs the kernels it always runs -- DropPath, dropout masks and the fp8 mode apply to frozen units as to any other,
 *             and logits / feats are bit-equal to the uncut plan's -- but the blocks before u write one shared set of activation buffers
 *             per stage and a ping-pong pair of fp32 stream buffers (as the blocks of an inference plan do), so nothing of theirs is kept.
 *             Units from u on keep their activations (or recompute them, cfg.recompute).
 *   backward  runs heads, tail, ... down to u inclusive and stops: no kernel of a unit before u is launched on any stream, no gradient
 *             slice of a parameter of such a unit is written or read (the pointers must still be valid addresses at the bind).  heads as
 *             the cut: the heads' weight and bias gradients only (dfeats is ignored, no final_norm backward).  At the cut unit a launch
 *             that only produces the unit's input gradient is skipped where it is a launch of its own (a conv block's depthwise data
 *             gradient); input gradients that fall out of a fused launch (a LayerNorm backward's dx) are still written, to scratch.
 *             A segment whose units all lie before u launches nothing and returns 0; it may still be called, in order, and the joins of
 *             what an earlier segment forked still happen in it.  lnx_plan_segment_params is unchanged.
 *   frozen parameters at or behind the cut: their gradient slices are unspecified after a backward (the fused launches write them).
 * LNX_FROZEN_PREFIX=0 in the environment, read by lnx_plan_create: lnx_plan_set_trainable checks and then ignores its mask (the A/B switch). */
int lnx_plan_num_units(const lnx_plan* p);
const char* lnx_plan_unit_name(const lnx_plan* p, int u);
int lnx_plan_param_unit(const lnx_plan* p, int i);
int lnx_plan_set_trainable(lnx_plan* p, const unsigned char* mask /* [lnx_plan_num_params] */);
int lnx_plan_first_trained_unit(const lnx_plan* p);
int lnx_plan_last_backward_units(const lnx_plan* p);

/* Input gradients (lnx_version 121): the backward continued through the stem to the image and through the metadata heads to the
 * metadata, what autograd gives the reference for `images.requires_grad_(True)` / `meta.requires_grad_(True)`.
 *   lnx_plan_set_input_grads(p, want_x, want_meta)   legal only between lnx_plan_create and lnx_plan_bind, in either order with
 *       lnx_plan_set_trainable (it may change lnx_plan_workspace_bytes); refused by name on an inference plan, after the bind, and
 *       want_meta on a plan without metadata components.  With a flag set the data path of the backward runs down to that source
 *       whatever the trainable mask: want_x moves the cut (lnx_plan_first_trained_unit) to the stem, want_meta to tokens_1 at the latest
 *       (the first unit that holds a metadata head; the RoPE stages, mid and everything behind them then run).  The units from the cut
 *       on run the launches they always run, so a frozen parameter behind the cut is treated as the fine-tuning contract above treats
 *       it: its gradient slice is unspecified and the caller hands no gradient out for it.  With a flag set lnx_plan_set_trainable
 *       accepts an all-zero mask (nothing trains, only the inputs are differentiated).  Both flags zero = the plan as created: the
 *       same workspace bytes, the same launches, the same bits.
 *   lnx_plan_input_grads(p)   bit 0: want_x, bit 1: want_meta (negative: NULL plan)
 *   lnx_plan_bind_input_grads(p, dx, dmeta)   where the NEXT lnx_plan_backward writes them; callable any time after the flags are set,
 *       before any backward; the pointers stay until the next call.  dx fp32 [B, Cin, H, W], 16-byte aligned, every element written
 *       (no pre-zeroing) in segment 3 behind the stem's weight gradient.  dmeta fp32 [B, sum(meta_dims)], every element written: the
 *       stage-4 heads write it and the stage-3 heads add to it (a fixed order: the heads of both stages run on one stream, the
 *       stage-4 heads first), and it is final after SEGMENT 2, where the stage-3 heads' backward is joined (as their parameter
 *       gradients are: lnx_plan_segment_params).  NULL skips that output for the backwards that follow; a pointer for an output whose
 *       flag is not set is refused.
 * lnx_plan_backward_into (GradNorm) never writes input gradients: its per-task backwards leave dx / dmeta untouched.
 * Recompute, fp8, DropPath-compacted, deterministic and fine-tuning plans take the same kernels: lnx_stem_dgrad where
 * lnx_stem_dgrad_ok, else lnx_gemm_nt on a transposed copy of the stem weight (kept in the operand arena of want_x plans only) +
 * lnx_col2im_stem; lnx_meta_input_grad for the metadata, one launch per stage with the one-launch chain and one per head on the
 * launch-by-launch path.  Second-order gradients (a graph through the backward) are out of scope. */
int lnx_plan_set_input_grads(lnx_plan* p, int want_x, int want_meta);
int lnx_plan_input_grads(const lnx_plan* p);
int lnx_plan_bind_input_grads(lnx_plan* p, float* dx, float* dmeta);

#ifdef __cplusplus
}
#endif
#endif /* LNX_H */
