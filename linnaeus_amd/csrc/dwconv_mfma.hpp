// Internal: MFMA variants of the depthwise 7x7 kernels (dwconv_mfma.hip), dispatched by the C-ABI entry points in
// dwconv.hip when an operand is bf16 (the production compute type).  Return value as the entry points.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/lnx.h"

bool lnx_dwconv_mfma_enabled();
// perm / nkeep: the list of lnx_dwconv7_fwd_kept / lnx_dwconv7_wgrad_kept, or NULL
int lnx_dwconv7_mfma_fwd(const lnx_dwconv_args* a, const int* perm, const int* nkeep, hipStream_t st);
int lnx_dwconv7_mfma_wgrad(const lnx_dwconv_wgrad_args* a, const int* perm, const int* nkeep, hipStream_t st);
int lnx_dwconv7_mfma_wgrad_walkers(int B, int H, int W, int C);  // workgroups per 16-channel block of that launch
// dwconv.hip: deterministic mode, after either weight-gradient kernel -- the walkers' partial sums in a->ws -> dw, db in walker order
int lnx_dwconv7_wgrad_fold(const lnx_dwconv_wgrad_args* a, int walkers, hipStream_t st);
