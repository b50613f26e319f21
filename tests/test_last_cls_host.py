"""The CLS-only last RoPE block on the host: which kernels its M = batch products take, from the functions lnx_gemm_nt and lnx_gemm_tn
themselves launch from (lnx_nt_dispatch, lnx_gemm_tn_query).  No GPU.  mFormerV1_sm stage 4: C = 768, hidden 3072, 52 tokens per sample."""
import ctypes as C

import pytest

from linnaeus_amd import _lib as L
from linnaeus_amd import ops

CH, HID, NTOK = 768, 3072, 52


def nt(M, N, K, form, lda=None, ldc=None):
    a = L.GemmArgs()
    one = C.c_void_p(16)  # (never dereferenced)
    a.dtype, a.M, a.N, a.K, a.lda, a.ldw, a.ldc = L.BF16, M, N, K, lda or K, K, ldc or N
    a.A = a.W = a.C = one
    if form in ("res_scaled", "res"):  # bias + fp32 residual (+ the sample's DropPath multiplier), fp32 output: proj / fc2
        a.bias = a.res = one
        a.ldres, a.out_f32 = a.ldc, 1
        if form == "res_scaled":
            a.rowscale, a.rows_per_sample = one, 1
    elif form == "fc1d":
        a.bias = a.c2 = one
        a.act, a.ldc2 = L.ACT_GELU_D, N
    elif form == "mul_aux":
        a.act, a.aux, a.ldaux = L.ACT_MUL_AUX, one, N
    return int(L.lib().lnx_nt_dispatch(C.byref(a)))


@pytest.mark.parametrize("B", [8, 128, 256])
def test_the_cls_row_products_leave_the_tile_kernels(B):
    ld = NTOK * CH  # row b of o / xin / xmid / the block output is row b * 52 of the token matrix
    # forward: proj and fc2 with a DropPath multiplier, fc1 with its two outputs -> the 128x128 kernel (the one-wave kernel has no
    # row-scale / second-output epilogue); without a multiplier (eval, or a call that drew none) proj and fc2 -> one wave per tile
    assert nt(B, CH, CH, "res_scaled", lda=ld, ldc=ld) == L.NT_KERNEL_V1
    assert nt(B, CH, HID, "res_scaled", ldc=ld) == L.NT_KERNEL_V1
    assert nt(B, HID, CH, "fc1d") == L.NT_KERNEL_V1
    assert nt(B, CH, CH, "res", lda=ld, ldc=ld) == L.NT_KERNEL_SKINNY and nt(B, CH, HID, "res", ldc=ld) == L.NT_KERNEL_SKINNY
    # backward: fc2's data gradient times GELU' -> 128x128; the plain fc1 and proj data gradients -> one wave per tile (proj's only
    # without a DropPath list for the attention call: with the list's device row count it stays on the 128x128 kernel)
    assert nt(B, HID, CH, "mul_aux") == L.NT_KERNEL_V1
    assert nt(B, CH, HID, "plain") == L.NT_KERNEL_SKINNY and nt(B, CH, CH, "plain", ldc=ld) == L.NT_KERNEL_SKINNY
    # the same products on all B * 52 rows are tile-kernel work from B = 24 on (tests/test_gpu_model.py's production-dispatch case)
    if B * NTOK >= 1024:
        assert nt(B * NTOK, HID, CH, "fc1d") not in (L.NT_KERNEL_V1, L.NT_KERNEL_SKINNY)


@pytest.mark.parametrize("B", [8, 128, 256])
@pytest.mark.parametrize("name,N,K,lda", [("fc2", CH, HID, HID), ("fc1", HID, CH, CH), ("proj", CH, CH, NTOK * CH)])
def test_the_cls_row_weight_gradients_are_one_workgroup_per_tile(B, name, N, K, lda):
    """M = B rows: the 128x128 kernel, one split (a contraction of at most 256 rows is below the four 64-row tiles a split is worth), so
    one contributor per element -- no partial tiles, no share of the block's reduce launch, and the same bits run to run."""
    q = ops.gemm_tn_query_shape(dtype=L.BF16, M=B, N=N, K=K, lda=lda, ws_floats=L.TN_WS_FLOATS)
    assert (q.kernel, q.rw, q.cw, q.splits, q.workspace) == (L.TN_KERNEL_V1, 128, 128, 1, 0)
    assert q.m_per_split == -(-B // 64) * 64
    full = ops.gemm_tn_query_shape(dtype=L.BF16, M=B * NTOK, N=N, K=K, ws_floats=L.TN_WS_FLOATS)
    if B * NTOK >= 4096 and B * NTOK % 64 == 0:
        assert full.kernel == L.TN_KERNEL_RING  # what the full block launches (tests/test_tn_dispatch_host.py)


def test_the_switch_is_exported():
    lib = L.lib()
    assert lib.lnx_version() >= 119
    prev = lib.lnx_set_last_cls(0)
    try:
        assert lib.lnx_set_last_cls(1) == 0 and lib.lnx_set_last_cls(-1) == 1
    finally:
        lib.lnx_set_last_cls(prev)
    assert lib.lnx_last_cls_blocks() >= 0
