"""Tensor-level wrappers over the C ABI (one function per entry point of include/lnx.h).

These take torch CUDA tensors only to obtain device pointers, sizes and the current HIP
stream; all arithmetic happens in liblnx_hip.so.  Used by the per-op parity tests and by
the model glue.  Nothing here has a CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from ._lib import F32, BF16  # noqa: F401

_TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16}


def code_of(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise L.LnxError(f"unsupported tensor dtype {t.dtype}")


def torch_dtype(code: int) -> torch.dtype:
    return _TORCH_DT[code]


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise L.LnxError("linnaeus_amd kernels need CUDA(HIP) tensors; there is no CPU fallback")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _map(m) -> L.RowMap:
    return L.RowMap(*(m or (0, 0, 0)))


def gemm_nt(A, W, out, *, M=None, N=None, K=None, lda=None, ldw=None, ldc=None, bias=None, act=L.ACT_NONE, aux=None, c2=None,
            gamma=None, rowscale=None, rows_per_sample=0, res=None, c_map=None, a_patch=None, c_patch=None, dtype=None, m_dev=None, perm=None):
    """out = epilogue(A . W^T); see lnx_gemm_args.  a_patch / c_patch = (Hin, Win, Cin).  m_dev / perm: compact rows (int32 device tensors)."""
    a = L.GemmArgs()
    a.dtype = dtype if dtype is not None else code_of(W)
    a.M = M if M is not None else A.shape[0]
    a.N = N if N is not None else W.shape[0]
    a.K = K if K is not None else W.shape[1]
    a.A, a.lda = _p(A), (lda if lda is not None else (A.stride(0) if a_patch is None else 0))
    a.W, a.ldw = _p(W), (ldw if ldw is not None else W.stride(0))
    a.C, a.ldc = _p(out), (ldc if ldc is not None else (out.stride(0) if c_patch is None else 0))
    a.out_f32 = int(out.dtype == torch.float32)
    if a_patch is not None:
        a.a_mode, a.Hin, a.Win, a.Cin = L.ADDR_PATCH2, *a_patch
    if c_patch is not None:
        a.c_mode, a.Hin, a.Win, a.Cin = L.ADDR_PATCH2, *c_patch
    a.c_map = _map(c_map)
    a.bias = _p(bias)
    a.c2, a.ldc2 = _p(c2), (c2.stride(0) if c2 is not None else 0)
    a.act, a.aux, a.ldaux = act, _p(aux), (aux.stride(0) if aux is not None else 0)
    a.gamma, a.rowscale, a.rows_per_sample = _p(gamma), _p(rowscale), rows_per_sample
    a.res, a.ldres = _p(res), ((res.stride(0) if c_patch is None else 0) if res is not None else 0)
    a.m_dev, a.perm = _p(m_dev), _p(perm)
    L.check(L.lib().lnx_gemm_nt(C.byref(a), _stream()), "lnx_gemm_nt")
    return out


def gemm_nt_group(problems, accumulate=False):
    """Several small bf16 products in one launch (lnx_gemm_nt_group).  problems: [(A, W, out, bias or None, res or None), ...];
    accumulate: out_0 = bias_0 + res_0 + sum_j A_j . W_j^T (the outputs / epilogue operands of the other entries are ignored: pass None)."""
    arr = (L.GemmArgs * len(problems))()
    for a, (A, W, out, bias, res) in zip(arr, problems):
        a.dtype = code_of(W)
        a.M, a.N, a.K = A.shape[0], W.shape[0], W.shape[1]
        a.A, a.lda, a.W, a.ldw = _p(A), A.stride(0), _p(W), W.stride(0)
        ref = out if out is not None else problems[0][2]
        a.C, a.ldc, a.out_f32 = _p(out), (out.stride(0) if out is not None else 0), int(ref.dtype == torch.float32)
        a.bias = _p(bias)
        a.res, a.ldres = _p(res), (res.stride(0) if res is not None else 0)
    if not L.lib().lnx_gemm_nt_group_ok(arr, len(problems), int(accumulate)):
        raise L.LnxError("lnx_gemm_nt_group: the problem list does not qualify")
    L.check(L.lib().lnx_gemm_nt_group(arr, len(problems), int(accumulate), _stream()), "lnx_gemm_nt_group")


def quantize_fp8(x, *, amax=None):
    """(x8, scale): x8 = e4m3fn(x * 448 / max|x|) as a torch.float8_e4m3fn tensor, scale = max|x| / 448 (device scalar).
    `amax`: a device scalar to use instead of this tensor's own maximum (delayed scaling)."""
    x2 = x.reshape(-1, x.shape[-1])
    if amax is None:
        amax = torch.zeros(1, device=x.device, dtype=torch.float32)
        L.check(L.lib().lnx_amax(_p(x2), code_of(x2), C.c_int64(x2.stride(0)), x2.shape[0], x2.shape[1], _p(amax), _stream()), "lnx_amax")
    y = torch.empty(x2.shape, device=x.device, dtype=torch.uint8)
    scale = torch.empty(1, device=x.device, dtype=torch.float32)
    L.check(L.lib().lnx_quantize_fp8(_p(x2), code_of(x2), C.c_int64(x2.stride(0)), x2.shape[0], x2.shape[1], _p(amax), _p(y), C.c_int64(y.stride(0)), _p(scale), _stream()),
            "lnx_quantize_fp8")
    return y.view(torch.float8_e4m3fn).reshape(x.shape), scale


def gemm_nt_fp8(A8, a_scale, W8, w_scale, out, *, bias=None, act=L.ACT_NONE, aux=None, c2=None, rowscale=None, rows_per_sample=0, res=None):
    """out = epilogue(a_scale * w_scale * A8 . W8^T) with e4m3 operands; see lnx_gemm_nt_fp8."""
    a = L.GemmArgs()
    a.dtype = L.BF16
    a.M, a.N, a.K = A8.shape[0], W8.shape[0], W8.shape[1]
    a.A, a.lda = _p(A8), A8.stride(0)
    a.W, a.ldw = _p(W8), W8.stride(0)
    a.C, a.ldc = _p(out), out.stride(0)
    a.out_f32 = int(out.dtype == torch.float32)
    a.bias = _p(bias)
    a.c2, a.ldc2 = _p(c2), (c2.stride(0) if c2 is not None else 0)
    a.act, a.aux, a.ldaux = act, _p(aux), (aux.stride(0) if aux is not None else 0)
    a.rowscale, a.rows_per_sample = _p(rowscale), rows_per_sample
    a.res, a.ldres = _p(res), (res.stride(0) if res is not None else 0)
    L.check(L.lib().lnx_gemm_nt_fp8(C.byref(a), _p(a_scale), _p(w_scale), _stream()), "lnx_gemm_nt_fp8")
    return out


def quantize_mxfp8(x):
    """(x8, scales): OCP MXFP8 -- e4m3fn elements with one power-of-two (E8M0) scale per 32 consecutive elements of a row.
    x8: torch.float8_e4m3fn [rows, cols]; scales: uint8 [cols/128, rows, 4] (byte j of [ks, r] = block 4 ks + j of row r),
    the layout lnx_gemm_nt_mxfp8 streams.  See lnx_quantize_mxfp8."""
    x2 = x.reshape(-1, x.shape[-1])
    rows, cols = x2.shape
    y = torch.empty(rows, cols, device=x.device, dtype=torch.uint8)
    sc = torch.empty(cols // 128, rows, 4, device=x.device, dtype=torch.uint8)
    L.check(L.lib().lnx_quantize_mxfp8(_p(x2), code_of(x2), C.c_int64(x2.stride(0)), rows, cols, _p(y), C.c_int64(y.stride(0)), _p(sc), _stream()),
            "lnx_quantize_mxfp8")
    return y.view(torch.float8_e4m3fn), sc


def dequantize_mxfp8(x8, scales):
    """fp32 tensor an MXFP8 pair stands for (tests, debugging)."""
    rows, cols = x8.shape
    e = scales.permute(1, 0, 2).reshape(rows, cols // 32).to(torch.float32) - 127.0
    return (x8.to(torch.float32).view(rows, cols // 32, 32) * torch.exp2(e).unsqueeze(-1)).view(rows, cols)


def gemm_nt_mxfp8(A8, a_scales, W8, w_scales, out, *, bias=None, act=L.ACT_NONE, aux=None, c2=None, rowscale=None, rows_per_sample=0, res=None,
                  c8=None, c8_scales=None):
    """out = epilogue(dequant(A8) . dequant(W8)^T) with MXFP8 operands (block scales applied by the matrix core); see lnx_gemm_nt_mxfp8."""
    a = L.GemmArgs()
    a.dtype = L.BF16
    a.M, a.N, a.K = A8.shape[0], W8.shape[0], W8.shape[1]
    a.A, a.lda = _p(A8), A8.stride(0)
    a.W, a.ldw = _p(W8), W8.stride(0)
    a.C, a.ldc = _p(out), out.stride(0)
    a.out_f32 = int(out.dtype == torch.float32)
    a.bias = _p(bias)
    a.c2, a.ldc2 = _p(c2), (c2.stride(0) if c2 is not None else 0)
    a.act, a.aux, a.ldaux = act, _p(aux), (aux.stride(0) if aux is not None else 0)
    a.rowscale, a.rows_per_sample = _p(rowscale), rows_per_sample
    a.res, a.ldres = _p(res), (res.stride(0) if res is not None else 0)
    if c8 is not None:
        a.c8, a.ldc8, a.c8_scales = _p(c8), c8.stride(0), _p(c8_scales)
    assert tuple(a_scales.shape) == (a.K // 128, a.M, 4) and tuple(w_scales.shape) == (a.K // 128, a.N, 4)
    L.check(L.lib().lnx_gemm_nt_mxfp8(C.byref(a), _p(a_scales), _p(w_scales), _stream()), "lnx_gemm_nt_mxfp8")
    return out


def _wgrad_args(dY, A, dW, *, M=None, N=None, K=None, lda=None, lddw=None, db=None, a_patch=None, k_perm_c=0, k_store=0, splits=0, dtype=None, ws=None,
                m_dev=None, defer=False) -> L.WgradArgs:
    a = L.WgradArgs()
    a.dtype = dtype if dtype is not None else code_of(dY)
    a.M = M if M is not None else dY.shape[0]
    a.N = N if N is not None else dY.shape[1]
    a.K = K if K is not None else (A.shape[1] if a_patch is None else 4 * a_patch[2])
    a.dY, a.lddy = _p(dY), dY.stride(0)
    a.A, a.lda = _p(A), (lda if lda is not None else (A.stride(0) if a_patch is None else 0))
    if a_patch is not None:
        a.a_mode, a.Hin, a.Win, a.Cin = L.ADDR_PATCH2, *a_patch
    a.dW, a.lddw = _p(dW), (lddw if lddw is not None else dW.stride(0))
    a.k_perm_c, a.db, a.splits, a.k_store = k_perm_c, _p(db), splits, k_store
    if ws is not None:
        a.ws, a.ws_floats = _p(ws), ws.numel()
    a.m_dev = _p(m_dev)
    a.defer = int(bool(defer))
    return a


def gemm_tn(dY, A, dW, **kw):
    """dW += dY^T . A (and db += colsum(dY)); see lnx_wgrad_args.  Keywords: M, N, K, lda, lddw, db, a_patch = (Hin, Win, Cin), k_perm_c, k_store, splits,
    dtype, ws, m_dev, defer.
    m_dev (optional device int32 tensor): the contraction stops at row min(M, m_dev[0]) -- see lnx_wgrad_args.m_dev.  ws (optional fp32 scratch): split-K partial tiles meet there and a second stage sums them in a fixed order; without it (or where
    it is too small) the splits meet in float atomics -- in deterministic mode the contraction is then split less, down to not at all.
    defer (with ws): the second stage is postponed to gemm_tn_flush()."""
    a = _wgrad_args(dY, A, dW, **kw)
    L.check(L.lib().lnx_gemm_tn(C.byref(a), _stream()), "lnx_gemm_tn")
    return dW


def gemm_tn_query(dY, A, dW, **kw) -> L.TnLaunch:
    """What gemm_tn(...) with the same arguments would launch (lnx_gemm_tn_query: kernel, tile form, splits, workspace or atomics); no device work."""
    a, out = _wgrad_args(dY, A, dW, **kw), L.TnLaunch()
    L.check(L.lib().lnx_gemm_tn_query(C.byref(a), C.byref(out)), "lnx_gemm_tn_query")
    return out


def gemm_tn_query_shape(*, dtype, M, N, K, lddy=None, lda=None, a_patch=None, k_perm_c=0, k_store=0, splits=0, ws_floats=0) -> L.TnLaunch:
    """lnx_gemm_tn_query from sizes alone (no tensors, no GPU): ws_floats > 0 stands for a workspace of that many floats."""
    epv = 4 if dtype == F32 else 8
    a, out = L.WgradArgs(), L.TnLaunch()
    a.dtype, a.M, a.N, a.K = dtype, M, N, K
    a.lddy = lddy if lddy is not None else -(-N // epv) * epv
    a.lda = lda if lda is not None else (K if a_patch is None else 0)
    if a_patch is not None:
        a.a_mode, a.Hin, a.Win, a.Cin = L.ADDR_PATCH2, *a_patch
    a.k_perm_c, a.splits, a.k_store = k_perm_c, splits, k_store
    if ws_floats > 0:
        a.ws, a.ws_floats = C.c_void_p(0x1000), ws_floats  # (never dereferenced: the query looks at "is there one, how large")
    L.check(L.lib().lnx_gemm_tn_query(C.byref(a), C.byref(out)), "lnx_gemm_tn_query")
    return out


def gemm_tn_flush():
    """Sums the partial tiles of this thread's deferred gemm_tn products into their dW / db (lnx_gemm_tn_flush)."""
    L.check(L.lib().lnx_gemm_tn_flush(_stream()), "lnx_gemm_tn_flush")


def _ln_args(x, w, b, y, eps, *, M=None, C_=None, ldx=None, ldy=None, x_map=None, y_map=None, add=None, ldadd=None, mean=None, rstd=None, y8=None, y8_scales=None,
             perm=None, m_dev=None, rows_per_sample=0):
    a = L.LnArgs()
    a.M = M if M is not None else x.shape[0]
    a.C = C_ if C_ is not None else x.shape[-1]
    a.eps = eps
    a.x, a.x_dtype, a.ldx, a.x_map = _p(x), code_of(x), (ldx if ldx is not None else x.stride(-2)), _map(x_map)
    a.w, a.b = _p(w), _p(b)
    a.y, a.y_dtype, a.ldy, a.y_map = _p(y), code_of(y), (ldy if ldy is not None else y.stride(-2)), _map(y_map)
    a.add, a.ldadd = _p(add), ((ldadd if ldadd is not None else add.stride(-2)) if add is not None else 0)
    a.mean, a.rstd = _p(mean), _p(rstd)
    if y8 is not None:
        a.y8, a.ldy8, a.y8_scales = _p(y8), y8.stride(0), _p(y8_scales)
    a.perm, a.m_dev, a.rows_per_sample = _p(perm), _p(m_dev), int(rows_per_sample)  # compact rows: see lnx_ln_args
    return a


def layernorm_fwd(x, w, b, y, eps, **kw):
    a = _ln_args(x, w, b, y, eps, **kw)
    L.check(L.lib().lnx_layernorm_fwd(C.byref(a), _stream()), "lnx_layernorm_fwd")
    return y


def layernorm_fwd_query(x, w, b, y, eps=0.0, **kw) -> L.LnLaunch:
    """The launch layernorm_fwd would make for the same arguments (lnx_layernorm_fwd_query: nothing runs)."""
    a, out = _ln_args(x, w, b, y, eps, **kw), L.LnLaunch()
    if L.lib().lnx_layernorm_fwd_query(C.byref(a), C.byref(out)) != 0:
        raise L.LnxError(f"lnx_layernorm_fwd_query refused: {L.lib().lnx_last_error().decode()}")
    return out


def _ln_bwd_args(dy, x, w, mean, rstd, dx, *, M=None, C_=None, lddy=None, ldx=None, lddx=None, dy_map=None, x_map=None, gin=None,
                 ldgin=None, dw=None, db=None, relu_mask=False, ws=None, dx2=None, lddx2=None, dx2_rowscale=None, dx2_rows_per_sample=0, dx2_8=None,
                 dx2_8_scales=None, defer=False, perm=None, m_dev=None, dx2_inv=None, dx2_nkeep=None):
    a = L.LnBwdArgs()
    a.M = M if M is not None else dy.shape[0]
    a.C = C_ if C_ is not None else x.shape[-1]
    a.dy, a.dy_dtype, a.lddy, a.dy_map = _p(dy), code_of(dy), (lddy if lddy is not None else dy.stride(-2)), _map(dy_map)
    a.x, a.x_dtype, a.ldx, a.x_map = _p(x), code_of(x), (ldx if ldx is not None else x.stride(-2)), _map(x_map)
    a.w, a.mean, a.rstd = _p(w), _p(mean), _p(rstd)
    a.gin, a.ldgin = _p(gin), ((ldgin if ldgin is not None else gin.stride(-2)) if gin is not None else 0)
    a.dx, a.dx_dtype, a.lddx = _p(dx), code_of(dx), (lddx if lddx is not None else dx.stride(-2))
    a.dw, a.db, a.relu_mask = _p(dw), _p(db), int(relu_mask)
    a.ws, a.ws_floats = _p(ws), (ws.numel() if ws is not None else 0)
    a.defer = int(defer)  # column-sum reduce postponed to layernorm_bwd_flush() (needs ws, one per pending call)
    if dx2 is not None:  # second output: rowscale[m // rows_per_sample] * dx in dx2's type (+ its MXFP8 copy)
        a.dx2, a.dx2_dtype, a.lddx2 = _p(dx2), code_of(dx2), (lddx2 if lddx2 is not None else dx2.stride(-2))
        a.dx2_rowscale, a.dx2_rows_per_sample = _p(dx2_rowscale), int(dx2_rows_per_sample)
        if dx2_8 is not None:
            a.dx2_8, a.dx2_8_scales, a.lddx2_8 = _p(dx2_8), _p(dx2_8_scales), dx2_8.stride(-2)
    if perm is not None or dx2_inv is not None:  # compact rows: see lnx_ln_bwd_args (rows per sample = dx2_rows_per_sample)
        a.dx2_rows_per_sample = int(dx2_rows_per_sample)
    a.perm, a.m_dev, a.dx2_inv, a.dx2_nkeep = _p(perm), _p(m_dev), _p(dx2_inv), _p(dx2_nkeep)
    return a


def layernorm_bwd(dy, x, w, mean, rstd, dx, **kw):
    a = _ln_bwd_args(dy, x, w, mean, rstd, dx, **kw)
    L.check(L.lib().lnx_layernorm_bwd(C.byref(a), _stream()), "lnx_layernorm_bwd")
    return dx


def layernorm_bwd_query(dy, x, w, mean, rstd, dx, **kw) -> L.LnLaunch:
    """The launch layernorm_bwd would make for the same arguments (lnx_layernorm_bwd_query: nothing runs)."""
    a, out = _ln_bwd_args(dy, x, w, mean, rstd, dx, **kw), L.LnLaunch()
    if L.lib().lnx_layernorm_bwd_query(C.byref(a), C.byref(out)) != 0:
        raise L.LnxError(f"lnx_layernorm_bwd_query refused: {L.lib().lnx_last_error().decode()}")
    return out


def layernorm_bwd_flush():
    L.check(L.lib().lnx_layernorm_bwd_flush(_stream()), "lnx_layernorm_bwd_flush")


def dwconv7(x, w49, bias, y, *, flip=False, res=None, perm=None, nkeep=None):
    """`perm` / `nkeep` (int32 device tensors of a lnx_drop_partition list): the kept samples only, include/lnx.h lnx_dwconv7_fwd_kept."""
    B, H, W, Cc = x.shape
    a = L.DwconvArgs()
    a.B, a.H, a.W, a.C = B, H, W, Cc
    a.x, a.x_dtype, a.w49, a.bias = _p(x), code_of(x), _p(w49), _p(bias)
    a.flip, a.res, a.y, a.y_dtype = int(flip), _p(res), _p(y), code_of(y)
    if perm is not None:
        L.check(L.lib().lnx_dwconv7_fwd_kept(C.byref(a), _p(perm), _p(nkeep), _stream()), "lnx_dwconv7_fwd_kept")
        return y
    L.check(L.lib().lnx_dwconv7_fwd(C.byref(a), _stream()), "lnx_dwconv7_fwd")
    return y


def dwconv7_wgrad(x, dy, dw, db, *, perm=None, nkeep=None):
    B, H, W, Cc = x.shape
    a = L.DwconvWgradArgs()
    a.B, a.H, a.W, a.C = B, H, W, Cc
    a.x, a.x_dtype, a.dy, a.dy_dtype, a.dw, a.db = _p(x), code_of(x), _p(dy), code_of(dy), _p(dw), _p(db)
    if L.is_deterministic():  # the walkers' partial sums, folded in walker order (the launcher says how many floats)
        ws = torch.empty(max(dwconv7_wgrad_ws_floats(B, H, W, Cc, a.x_dtype, a.dy_dtype), 1), device=x.device, dtype=torch.float32)
        a.ws, a.ws_floats = _p(ws), ws.numel()
    if perm is not None:
        L.check(L.lib().lnx_dwconv7_wgrad_kept(C.byref(a), _p(perm), _p(nkeep), _stream()), "lnx_dwconv7_wgrad_kept")
        return
    L.check(L.lib().lnx_dwconv7_wgrad(C.byref(a), _stream()), "lnx_dwconv7_wgrad")


def dwconv7_wgrad_ws_floats(B, H, W, Cc, x_dtype, dy_dtype) -> int:
    return int(L.lib().lnx_dwconv7_wgrad_ws_floats(B, H, W, Cc, x_dtype, dy_dtype))


def rope_cos_table(freqs, H, W, out=None, dsin=None):
    """cos(theta) table [H*W, heads, head_dim/2] of freqs [2, heads, head_dim/2]; `dsin` (optional, [2, H*W, heads, head_dim/2])
    receives -t_x sin(theta), -t_y sin(theta)."""
    heads, half = freqs.shape[1], freqs.shape[2]
    if out is None:
        out = torch.empty(H * W, heads, half, device=freqs.device, dtype=torch.float32)
    L.check(L.lib().lnx_rope_cos_table_hd(_p(freqs), heads, 2 * half, H, W, _p(out), _p(dsin) if dsin is not None else None, _stream()),
            "lnx_rope_cos_table_hd")
    return out


def rope_cossin_table(freqs, H, W):
    """(cos(theta), sin(theta)) tables, each [H*W, heads, head_dim/2], of freqs [2, heads, head_dim/2]: the operands of the rotate
    form of attn_fwd / attn_bwd."""
    heads, half = freqs.shape[1], freqs.shape[2]
    cos = torch.empty(H * W, heads, half, device=freqs.device, dtype=torch.float32)
    sin = torch.empty_like(cos)
    L.check(L.lib().lnx_rope_cossin_table_hd(_p(freqs), heads, 2 * half, H, W, _p(cos), _p(sin), None, _stream()), "lnx_rope_cossin_table_hd")
    return cos, sin


def rope_cos_tables(entries):
    """The tables of several blocks in one launch per head_dim: entries = [(freqs [2,heads,head_dim/2], H, W, cos_out, dsin_out or None), ...];
    a sixth element, sin_out, makes the entry a rotate-mode table (sin(theta) beside cos(theta))."""
    arr = (L.RopeTable * len(entries))()
    for t, (freqs, H, W, out, dsin, *rest) in zip(arr, entries):
        t.freqs, t.cos_out, t.dsin_out = _p(freqs), _p(out), _p(dsin) if dsin is not None else None
        t.heads, t.H, t.W, t.head_dim = freqs.shape[1], H, W, 2 * freqs.shape[2]
        if rest and rest[0] is not None:
            t.rope_mode, t.sin_out = L.ROPE_ROTATE, _p(rest[0])
    L.check(L.lib().lnx_rope_cos_tables(arr, len(entries), _stream()), "lnx_rope_cos_tables")


def attn_bwd_ws_floats(B, N, heads, head_dim=64):
    fn = L.lib().lnx_attn_bwd_ws_floats_hd
    fn.restype = C.c_int64
    return int(fn(B, N, heads, head_dim))


def _head_dim(qkv, heads, head_dim):
    """head_dim from qkv [..., 3*heads*head_dim] unless given (64 for a flat qkv, as before head_dim was an argument)"""
    if head_dim is not None:
        return int(head_dim)
    return qkv.shape[-1] // (3 * heads) if qkv.dim() >= 2 and qkv.shape[-1] % (3 * heads) == 0 else 64


def attn_fwd(qkv, cos_tab, o, lse, B, N, E, heads, *, drop_mask=None, drop_rate=0.0, head_dim=None, sin_tab=None, nkeep=None):
    """sin_tab (the second table of rope_cossin_table): the rotate form -- q and k pairs rotated by theta instead of scaled by cos(theta)."""
    a = L.AttnArgs()
    if sin_tab is not None:
        a.rope_mode, a.sin_tab = L.ROPE_ROTATE, _p(sin_tab)
    a.dtype, a.B, a.N, a.E, a.heads = code_of(qkv), B, N, E, heads
    a.head_dim = _head_dim(qkv, heads, head_dim)
    a.qkv, a.cos_tab, a.o, a.lse = _p(qkv), _p(cos_tab), _p(o), _p(lse)
    if drop_mask is not None:
        a.drop_mask, a.drop_inv_keep = _p(drop_mask), 1.0 / (1.0 - drop_rate)
    if nkeep is not None:  # compact rows (int32 device tensor): samples b >= nkeep[0] are skipped
        L.check(L.lib().lnx_attn_fwd_compact(C.byref(a), _p(nkeep), _stream()), "lnx_attn_fwd_compact")
        return
    L.check(L.lib().lnx_attn_fwd(C.byref(a), _stream()), "lnx_attn_fwd")


def attn_bwd(qkv, cos_tab, o, lse, d_o, dqkv, delta, B, N, E, heads, *, dsin=None, dfreqs=None, drop_mask=None, drop_rate=0.0, defer_freqs=False,
             head_dim=None, sin_tab=None, grid_w=0, nkeep=None):
    """dq/dk/dv into dqkv; with image tokens (E < N) also dfreqs [2, heads, head_dim/2] += the gradient of the RoPE frequencies
    (`dsin` = the second table of rope_cos_table).  head_dim: from qkv's width unless given.  defer_freqs: the fold into dfreqs
    waits for attn_bwd_flush(); the returned workspace (and dfreqs) must be kept alive until then.
    Rotate form: sin_tab (rope_cossin_table) and grid_w (the W of the tables) instead of dsin."""
    a = L.AttnBwdArgs()
    if sin_tab is not None:
        a.rope_mode, a.sin_tab, a.grid_w, a.dfreqs = L.ROPE_ROTATE, _p(sin_tab), int(grid_w), _p(dfreqs) if dfreqs is not None else None
    a.dtype, a.B, a.N, a.E, a.heads = code_of(qkv), B, N, E, heads
    a.head_dim = _head_dim(qkv, heads, head_dim)
    a.qkv, a.cos_tab, a.o, a.lse = _p(qkv), _p(cos_tab), _p(o), _p(lse)
    ws = torch.empty(max(attn_bwd_ws_floats(B, N, heads, a.head_dim), 1), device=qkv.device, dtype=torch.float32)
    a.d_o, a.dqkv, a.freq_ws, a.delta = _p(d_o), _p(dqkv), _p(ws), _p(delta)
    if dsin is not None:
        a.dsin_tab, a.dfreqs = _p(dsin), _p(dfreqs)
    if drop_mask is not None:
        a.drop_mask, a.drop_inv_keep = _p(drop_mask), 1.0 / (1.0 - drop_rate)
    a.defer_freqs = int(bool(defer_freqs))
    if nkeep is not None:  # compact rows, as attn_fwd (kept alive by the caller until attn_bwd_flush when the fold is postponed)
        L.check(L.lib().lnx_attn_bwd_compact(C.byref(a), _p(nkeep), C.c_int64(ws.numel()), _stream()), "lnx_attn_bwd_compact")
        return ws
    L.check(L.lib().lnx_attn_bwd_sized(C.byref(a), C.c_int64(ws.numel()), _stream()), "lnx_attn_bwd")
    return ws


def attn_bwd_flush():
    """Fold every postponed freqs gradient of this thread (one launch)."""
    L.check(L.lib().lnx_attn_bwd_flush(_stream()), "lnx_attn_bwd_flush")


def im2col_stem(x, patches):
    B, Cin, H, W = x.shape
    L.check(L.lib().lnx_im2col_stem(_p(x), B, Cin, H, W, _p(patches), code_of(patches), patches.stride(0), _stream()), "lnx_im2col_stem")


def stem_fwd(x, w, bias, ln_w, ln_b, y, *, patches=None, pre=None, mean=None, rstd=None, eps=1e-6):
    """conv 4x4/4 + bias (bf16 output) + channels-first LayerNorm in one launch: x fp32 [B, Cin, H, W], w bf16 [Cout, 64]"""
    a = L.StemArgs()
    a.x, a.w, a.bias, a.ln_w, a.ln_b = _p(x), _p(w), _p(bias), _p(ln_w), _p(ln_b)
    a.patches, a.pre, a.y, a.mean, a.rstd = _p(patches), _p(pre), _p(y), _p(mean), _p(rstd)
    a.B, a.Cin, a.H, a.W = x.shape
    a.Cout, a.eps = w.shape[0], eps
    L.check(L.lib().lnx_stem_fwd(C.byref(a), _stream()), "lnx_stem_fwd")


def stem_dgrad_ok(dtype_code: int, Cin: int, H: int, W: int, Cout: int) -> bool:
    return bool(L.lib().lnx_stem_dgrad_ok(dtype_code, Cin, H, W, Cout))


def stem_dgrad(dy, w, dx, *, Cout=None):
    """dx fp32 [B, Cin, H, W] = unpatchify(dy . w): the transpose of Conv2d(Cin, Cout, 4, 4).  dy [M, ldy] (bf16 or fp32, the first Cout
    columns count; ldy = dy.stride(0)), w [Cout, 64] of dy's dtype.  Every element of dx is written."""
    a = L.StemDgradArgs()
    a.dtype = code_of(dy)
    a.B, a.Cin, a.H, a.W = dx.shape
    a.Cout = Cout if Cout is not None else w.shape[0]
    a.dy, a.ldy, a.w, a.dx = _p(dy), dy.stride(0), _p(w), _p(dx)
    L.check(L.lib().lnx_stem_dgrad(C.byref(a), _stream()), "lnx_stem_dgrad")


def col2im_stem(patches, dx):
    """The inverse of im2col_stem: patches [M, ldp] (column k = c*16 + kh*4 + kw) -> dx fp32 [B, Cin, H, W], every element written."""
    B, Cin, H, W = dx.shape
    L.check(L.lib().lnx_col2im_stem(_p(patches), code_of(patches), patches.stride(0), B, Cin, H, W, _p(dx), _stream()), "lnx_col2im_stem")


def meta_input_grad(heads, dmeta, *, accumulate=False):
    """dmeta[b, off + j] (+)= sum_o dp0[b, o] w0[o, j] for every (dp0 [B, C], w0 [C, ldw0 >= dim], dim, off) of `heads` (at most
    LNX_MAX_META, disjoint column ranges), fp32, one launch, a fixed summation order."""
    arr = (L.MetaInputGradArgs * max(len(heads), 1))()
    for a, (dp0, w0, dim, off) in zip(arr, heads):
        a.B, a.C = dp0.shape
        a.dim, a.off = dim, off
        a.dp0, a.lddp0, a.w0, a.ldw0 = _p(dp0), dp0.stride(0), _p(w0), w0.stride(0)
    L.check(L.lib().lnx_meta_input_grad(arr, len(heads), _p(dmeta), dmeta.stride(0), int(bool(accumulate)), _stream()), "lnx_meta_input_grad")


def scale_cast(inp, out, M, Cc, *, ldin=None, in_map=None, rowscale=None, rows_per_sample=0, ldout=None):
    L.check(L.lib().lnx_scale_cast(_p(inp), C.c_int64(ldin if ldin is not None else inp.stride(-2)), _map(in_map), _p(rowscale), rows_per_sample,
                                   _p(out), code_of(out), C.c_int64(ldout if ldout is not None else out.stride(-2)), M, Cc, _stream()), "lnx_scale_cast")


def scale_cast_compact(inp, out, M, Cc, *, perm, m_dev, rows_per_sample, rowscale=None, ldin=None, ldout=None):
    """out[m', :] = rowscale[b] * inp[b * rows_per_sample + m' % rows_per_sample, :], b = perm[m' // rows_per_sample], for m' < min(M, m_dev[0])"""
    L.check(L.lib().lnx_scale_cast_compact(_p(inp), C.c_int64(ldin if ldin is not None else inp.stride(-2)), _p(rowscale), rows_per_sample, _p(perm), _p(m_dev),
                                           _p(out), code_of(out), C.c_int64(ldout if ldout is not None else out.stride(-2)), M, Cc, _stream()), "lnx_scale_cast_compact")


def copy_dropped_rows(src, dst, *, perm, nkeep, rows_per_sample, Cc=None, ld=None):
    """dst rows of the samples behind nkeep[0] in perm = src rows, bit for bit: rows perm[j] * rows_per_sample + t, j >= nkeep[0]; both fp32 with
    leading dimension ld"""
    L.check(L.lib().lnx_copy_dropped_rows(_p(src), _p(dst), C.c_int64(ld if ld is not None else dst.stride(-2)), _p(perm), _p(nkeep), perm.numel(), rows_per_sample,
                                          Cc if Cc is not None else dst.shape[-1], _stream()), "lnx_copy_dropped_rows")


class DropLists:
    """The DropPath compaction lists of lnx_drop_partition as views of one int32 tensor [n_calls, 2 B + 2]."""

    def __init__(self, lists: torch.Tensor, B: int):
        self.lists, self.B = lists, B

    def nkeep(self, c):
        return self.lists[c, 0:1]

    def m_dev(self, c):
        return self.lists[c, 1:2]

    def perm(self, c):
        return self.lists[c, 2:2 + self.B]

    def inv(self, c):
        return self.lists[c, 2 + self.B:2 + 2 * self.B]


def drop_partition(scales: torch.Tensor, rows_per_sample=None, call_mask=None) -> DropLists:
    """scales [n_calls, B] fp32 (device): one list per call (call_mask: host sequence of 0 / 1, calls with 0 are left unwritten)."""
    n, B = scales.shape
    lists = torch.zeros((n, L.drop_list_ints(B)), device=scales.device, dtype=torch.int32)
    rps = (C.c_int * n)(*[int(r) for r in rows_per_sample]) if rows_per_sample is not None else None
    mask = bytes(bytearray(int(bool(m)) for m in call_mask)) if call_mask is not None else None
    L.check(L.lib().lnx_drop_partition(_p(scales.contiguous()), n, B, mask, rps, _p(lists), _stream()), "lnx_drop_partition")
    return DropLists(lists, B)


def layerscale_bwd(g, z, gamma, rowscale, rows_per_sample, dz, dgamma, M, Cc):
    if L.is_deterministic():  # the workgroups' dgamma partial sums, folded in workgroup order
        ws = torch.empty(max(int(L.lib().lnx_layerscale_bwd_ws_floats(M, Cc)), 1), device=g.device, dtype=torch.float32)
        L.check(L.lib().lnx_layerscale_bwd_ws(_p(g), _p(z), code_of(z), _p(gamma), _p(rowscale), rows_per_sample, _p(dz), _p(dgamma), M, Cc, _p(ws),
                                              C.c_int64(ws.numel()), _stream()), "lnx_layerscale_bwd_ws")
        return
    L.check(L.lib().lnx_layerscale_bwd(_p(g), _p(z), code_of(z), _p(gamma), _p(rowscale), rows_per_sample, _p(dz), _p(dgamma), M, Cc, _stream()),
            "lnx_layerscale_bwd")


def fill_rows(vec, out, ldout, row_map, M, Cc):
    L.check(L.lib().lnx_fill_rows(_p(vec), _p(out), C.c_int64(ldout), _map(row_map), M, Cc, _stream()), "lnx_fill_rows")


def colsum_rows(inp, ldin, row_map, out, M, Cc):
    L.check(L.lib().lnx_colsum_rows(_p(inp), C.c_int64(ldin), _map(row_map), _p(out), M, Cc, _stream()), "lnx_colsum_rows")


def agg2_fwd(a, b, w2, bias1, out, M, Cc):
    L.check(L.lib().lnx_agg2_fwd(_p(a), _p(b), _p(w2), _p(bias1), _p(out), M, Cc, _stream()), "lnx_agg2_fwd")


def agg2_bwd(dout, a, b, w2, da, db, dw2, dbias1, M, Cc):
    L.check(L.lib().lnx_agg2_bwd(_p(dout), _p(a), _p(b), _p(w2), _p(da), _p(db), _p(dw2), _p(dbias1), M, Cc, _stream()), "lnx_agg2_bwd")


def pack_meta(meta, off, dim, out):
    L.check(L.lib().lnx_pack_meta(_p(meta), meta.shape[1], off, dim, _p(out), code_of(out), meta.shape[0], _stream()), "lnx_pack_meta")


def convmlp_fwd(ln, w1, b1, w2, b2, gamma, x, out, *, rowscale=None, rows_per_sample=0, z=None, y=None, ln_w=None, ln_b=None, ln_eps=1e-6,
                ln_out=None, mean=None, rstd=None, perm=None, m_dev=None):
    """`y` given (and `ln` None): the kernel applies the block LayerNorm (ln_w, ln_b, ln_eps) to y itself and writes ln_out / mean / rstd.
    `perm` / `m_dev` (int32 device tensors of a lnx_drop_partition list): compact rows, include/lnx.h lnx_convmlp_args."""
    a = L.ConvMlpArgs()
    src = ln if y is None else y
    a.dtype, a.M, a.C = code_of(src), src.shape[0], src.shape[1]
    a.ln, a.w1, a.b1, a.w2, a.b2, a.gamma = _p(ln), _p(w1), _p(b1), _p(w2), _p(b2), _p(gamma)
    a.rowscale, a.rows_per_sample, a.x, a.out, a.z = _p(rowscale), rows_per_sample, _p(x), _p(out), _p(z)
    a.y, a.ln_w, a.ln_b, a.ln_eps, a.ln_out, a.mean, a.rstd = _p(y), _p(ln_w), _p(ln_b), ln_eps, _p(ln_out), _p(mean), _p(rstd)
    a.perm, a.m_dev = _p(perm), _p(m_dev)
    L.check(L.lib().lnx_convmlp_fwd(C.byref(a), _stream()), "lnx_convmlp_fwd")
    return out


def layerscale_apply_wgrad(s, t, w, b, gamma, dw, db, dgamma):
    """dw[c, :] += gamma[c] s[c, :], db[c] += gamma[c] t[c], dgamma[c] += sum_k w[c, k] s[c, k] + b[c] t[c]  (include/lnx.h: the
    LayerScale gradient without z; s / t = the pwconv2 weight / bias gradient of dY = rowscale * g, in zeroed scratch)."""
    L.check(L.lib().lnx_layerscale_apply_wgrad(_p(s), _p(t), C.c_int64(s.stride(0)), _p(w), _p(b), C.c_int64(w.stride(0)), _p(gamma), _p(dw), _p(db),
                                               C.c_int64(dw.stride(0)), _p(dgamma), w.shape[0], w.shape[1], _stream()), "lnx_layerscale_apply_wgrad")


def convmlp_bwd(g, ln, z, w1, b1, w2t, w1t, gamma, act, dh, dz, dln, dgamma, *, rowscale=None, rows_per_sample=0, y=None, ln_w=None, mean=None,
                rstd=None, d_ln_w=None, d_ln_b=None, ws=None, dz_plain=False, ln_defer=False, perm=None, m_dev=None):
    """`y` given: the LayerNorm backward runs in the kernel too -- `dln` receives the gradient wrt y, d_ln_w / d_ln_b are accumulated."""
    a = L.ConvMlpBwdArgs()
    a.dtype, a.M, a.C = code_of(ln), ln.shape[0], ln.shape[1]
    a.g, a.ln, a.z, a.w1, a.b1, a.w2t, a.w1t, a.gamma = _p(g), _p(ln), _p(z), _p(w1), _p(b1), _p(w2t), _p(w1t), _p(gamma)
    a.rowscale, a.rows_per_sample = _p(rowscale), rows_per_sample
    a.act, a.dh, a.dz, a.dln, a.dgamma = _p(act), _p(dh), _p(dz), _p(dln), _p(dgamma)
    a.y, a.ln_w, a.mean, a.rstd, a.d_ln_w, a.d_ln_b = _p(y), _p(ln_w), _p(mean), _p(rstd), _p(d_ln_w), _p(d_ln_b)
    a.ws, a.ws_floats = _p(ws), (ws.numel() if ws is not None else 0)
    a.dz_plain, a.ln_defer = int(dz_plain), int(ln_defer)
    a.perm, a.m_dev = _p(perm), _p(m_dev)
    L.check(L.lib().lnx_convmlp_bwd(C.byref(a), _stream()), "lnx_convmlp_bwd")


# ---- metadata-head chains in one launch per direction (metahead.hip; reference mFormerV1.py:282-311, res_norm_layer.py:23-30) ----
def _meta_head_buffers(B, C_, dev):
    f = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
    return {"t0": f(B, 16), "h0": f(B, C_), "x": f(B, C_), "h1": f(B, C_), "n1": f(B, C_), "h2": f(B, C_),
            "m0": f(B), "r0": f(B), "m1": f(B), "r1": f(B), "m2": f(B), "r2": f(B)}


def meta_heads_fwd(meta, heads, tok, eps=1e-5):
    """heads: list of dicts with `off`, `dim`, `slot` (token row of a sample, 1 + m) and the parameters `w0` [C, dim], `b0`, `ln0_w`, `ln0_b`,
    `w1`, `b1`, `ln1_w`, `ln1_b`, `w2`, `b2`, `ln2_w`, `ln2_b`.  tok: [B, N, C] fp32, row `slot` of every sample is written.
    Returns the per-head activation dicts the backward needs."""
    B = meta.shape[0]
    arr = (L.MetaHeadArgs * len(heads))()
    keep, saved = [], []
    for i, h in enumerate(heads):
        C_ = h["w1"].shape[0]
        w0p = torch.zeros(C_, 16, device=meta.device)
        w0p[:, :h["dim"]] = h["w0"]
        bufs = _meta_head_buffers(B, C_, meta.device)
        t = tok[i] if isinstance(tok, (list, tuple)) else tok
        a = arr[i]
        a.B, a.C, a.dim, a.off, a.meta, a.meta_width, a.eps = B, C_, h["dim"], h["off"], _p(meta), meta.shape[1], eps
        a.w0, a.ldw0, a.b0, a.ln0_w, a.ln0_b = _p(w0p), 16, _p(h["b0"]), _p(h["ln0_w"]), _p(h["ln0_b"])
        a.w1, a.ldw1, a.b1, a.ln1_w, a.ln1_b = _p(h["w1"]), C_, _p(h["b1"]), _p(h["ln1_w"]), _p(h["ln1_b"])
        a.w2, a.ldw2, a.b2, a.ln2_w, a.ln2_b = _p(h["w2"]), C_, _p(h["b2"]), _p(h["ln2_w"]), _p(h["ln2_b"])
        for k_, v in bufs.items():
            setattr(a, k_, _p(v))
        a.tok, a.tok_row_stride, a.tok_row_offset = _p(t), t.shape[1] * C_, h["slot"] * C_
        keep.append(w0p)
        saved.append(bufs)
    L.check(L.lib().lnx_meta_heads_fwd(arr, len(heads), _stream()), "lnx_meta_heads_fwd")
    return saved


def meta_heads_bwd(g, heads, saved, grads):
    """g: [B, N, C] gradient of the token matrix (or a list, one per head); grads: per head a dict of fp32 tensors (torch layouts) that are ADDED to."""
    arr = (L.MetaHeadBwdArgs * len(heads))()
    keep = []
    for i, (h, sv, gr) in enumerate(zip(heads, saved, grads)):
        C_ = h["w1"].shape[0]
        gi = g[i] if isinstance(g, (list, tuple)) else g
        B = gi.shape[0]
        w1t, w2t = h["w1"].t().contiguous(), h["w2"].t().contiguous()
        dp = [torch.empty(B, C_, device=gi.device) for _ in range(3)]
        part = torch.empty(L.lib().lnx_meta_heads_bwd_part_floats(B, C_), device=gi.device)
        a = arr[i]
        a.B, a.C, a.dim = B, C_, h["dim"]
        a.g, a.g_row_stride, a.g_row_offset = _p(gi), gi.shape[1] * C_, h["slot"] * C_
        a.w1t, a.ldw1t, a.w2t, a.ldw2t = _p(w1t), C_, _p(w2t), C_
        a.ln0_w, a.ln1_w, a.ln2_w = _p(h["ln0_w"]), _p(h["ln1_w"]), _p(h["ln2_w"])
        for k_, v in sv.items():
            setattr(a, k_, _p(v))
        a.dp2, a.dp1, a.dp0, a.part = _p(dp[0]), _p(dp[1]), _p(dp[2]), _p(part)
        for k_ in ("w0", "b0", "ln0_w", "ln0_b", "w1", "b1", "ln1_w", "ln1_b", "w2", "b2", "ln2_w", "ln2_b"):
            setattr(a, "d_" + k_, _p(gr[k_]))
        keep += [w1t, w2t, part] + dp
    L.check(L.lib().lnx_meta_heads_bwd(arr, len(heads), _stream()), "lnx_meta_heads_bwd")
    torch.cuda.current_stream().synchronize()  # (the scratch tensors above die with this frame)


def metrics_table_sizes(n_tasks: int, n_bins0: int = 0, n_bins1: int = 0) -> Tuple[int, int]:
    """Lengths of the int64 counts / double sums tables of metrics_update (lnx_metrics_table_sizes)."""
    nc, ns = C.c_int64(), C.c_int64()
    L.check(L.lib().lnx_metrics_table_sizes(n_tasks, n_bins0, n_bins1, C.byref(nc), C.byref(ns)), "lnx_metrics_table_sizes")
    return nc.value, ns.value


def metrics_update(logits, targets, counts, sums, *, num_classes=None, is_null=None, losses=None, subset_ids=(), n_bins=()):
    """One lnx_metrics_update launch: ADDS a batch's counters to counts (int64) / sums (float64).  logits: per task [B, >= C] rows of one
    dtype (fp32 / bf16) with unit column stride (padded views welcome: stride(0) is the ld), tasks in ascending rank order; targets: per
    task int64 [B]; num_classes: per task C (default: the logits' width); is_null / losses: per task uint8 [B] / fp32 [B] or None;
    subset_ids: up to two int64 [B] with their n_bins."""
    T = len(logits)
    if not 1 <= T <= L.METRICS_MAX_TASKS or len(targets) != T:
        raise L.LnxError(f"metrics_update: {T} tasks (1..{L.METRICS_MAX_TASKS}), {len(targets)} targets")
    a = L.MetricsArgs()
    a.dtype, a.B, a.n_tasks = code_of(logits[0]), logits[0].shape[0], T
    for t in range(T):
        x, tg = logits[t], targets[t]
        nul = is_null[t] if is_null is not None else None
        ls = losses[t] if losses is not None else None
        if x.dim() != 2 or x.shape[0] != a.B or code_of(x) != a.dtype or (x.shape[1] > 1 and x.stride(1) != 1):
            raise L.LnxError(f"metrics_update: task {t} logits must be [B, C] rows of one dtype with unit column stride, got {tuple(x.shape)} {x.dtype} strides {x.stride()}")
        if tg.dtype != torch.int64 or tg.shape != (a.B,) or not tg.is_contiguous():
            raise L.LnxError(f"metrics_update: task {t} target must be contiguous int64 [B]")
        if nul is not None and (nul.dtype not in (torch.uint8, torch.bool) or nul.shape != (a.B,) or not nul.is_contiguous()):
            raise L.LnxError(f"metrics_update: task {t} is_null must be contiguous uint8 / bool [B]")
        if ls is not None and (ls.dtype != torch.float32 or ls.shape != (a.B,) or not ls.is_contiguous()):
            raise L.LnxError(f"metrics_update: task {t} loss must be contiguous fp32 [B]")
        k = a.task[t]
        k.logits, k.ld, k.C = _p(x), (x.stride(0) if a.B > 1 else x.shape[1]), (num_classes[t] if num_classes is not None else x.shape[1])
        k.target, k.is_null, k.loss = _p(tg), _p(nul), _p(ls)
    for s, (ids, nb) in enumerate(zip(subset_ids, n_bins)):
        if ids is None:
            continue
        if ids.dtype != torch.int64 or ids.shape != (a.B,) or not ids.is_contiguous():
            raise L.LnxError(f"metrics_update: subset ids {s} must be contiguous int64 [B]")
        a.subset_ids[s], a.n_bins[s] = ids.data_ptr(), nb
    nc, ns = metrics_table_sizes(T, a.n_bins[0], a.n_bins[1])
    if counts.dtype != torch.int64 or sums.dtype != torch.float64 or counts.numel() < nc or sums.numel() < ns or not (counts.is_contiguous() and sums.is_contiguous()):
        raise L.LnxError(f"metrics_update: tables must be contiguous int64 [>= {nc}] / float64 [>= {ns}]")
    a.counts, a.sums = _p(counts), _p(sums)
    L.check(L.lib().lnx_metrics_update(C.byref(a), _stream()), "lnx_metrics_update")


def predict_topk(logits, parents, *, K, null_index=0, id_maps=None, k_per_sample=None, consistency=True, num_classes=None, out=None):
    """One lnx_predict launch: the final top-K (id, probability) lists of every sample and task.  logits: per task [B, >= C] rows of one
    dtype (fp32 / bf16) with unit column stride (padded views welcome: stride(0) is the ld), tasks FINEST FIRST; parents: per task int32
    [C] (class -> class of the next coarser task, -1 = none), None for the coarsest; null_index: an int or per task an int / None
    (= the task cannot be nullified); id_maps: per task int64 [C] or None; k_per_sample: int32 [B] or None; num_classes: per task C
    (default: the logits' width); out: (ids, probs, count, flags) to write into instead of new tensors.
    Returns ids int64 [B, T, K], probs fp32 [B, T, K], count int32 [B, T], flags int32 [B, T]; never synchronises."""
    T = len(logits)
    if not 1 <= T <= L.METRICS_MAX_TASKS or len(parents) != T:
        raise L.LnxError(f"predict_topk: {T} tasks (1..{L.METRICS_MAX_TASKS}), {len(parents)} parent tables")
    nulls = list(null_index) if isinstance(null_index, (list, tuple)) else [null_index] * T
    if len(nulls) != T or (id_maps is not None and len(id_maps) != T):
        raise L.LnxError(f"predict_topk: {T} tasks need {T} null indices / id maps")
    a = L.PredictArgs()
    a.dtype, a.B, a.n_tasks, a.K, a.consistency = code_of(logits[0]), logits[0].shape[0], T, int(K), int(bool(consistency))
    dev = logits[0].device
    for t in range(T):
        x, par = logits[t], parents[t]
        ids = id_maps[t] if id_maps is not None else None
        if x.dim() != 2 or x.shape[0] != a.B or code_of(x) != a.dtype or (x.shape[1] > 1 and x.stride(1) != 1):
            raise L.LnxError(f"predict_topk: task {t} logits must be [B, C] rows of one dtype with unit column stride, got {tuple(x.shape)} {x.dtype} strides {x.stride()}")
        Ct = int(num_classes[t]) if num_classes is not None else x.shape[1]
        if Ct > x.shape[1]:
            raise L.LnxError(f"predict_topk: task {t} has {x.shape[1]} logit columns, {Ct} classes")
        if par is not None and (par.dtype != torch.int32 or par.shape != (Ct,) or not par.is_contiguous()):
            raise L.LnxError(f"predict_topk: task {t} parent table must be contiguous int32 [{Ct}]")
        if ids is not None and (ids.dtype != torch.int64 or ids.shape != (Ct,) or not ids.is_contiguous()):
            raise L.LnxError(f"predict_topk: task {t} id map must be contiguous int64 [{Ct}]")
        k = a.task[t]
        k.logits, k.ld, k.C = _p(x), (x.stride(0) if a.B > 1 else x.shape[1]), Ct
        k.parent, k.id_map, k.null_index = _p(par), _p(ids), (-1 if nulls[t] is None else int(nulls[t]))
    if k_per_sample is not None:
        if k_per_sample.dtype != torch.int32 or k_per_sample.shape != (a.B,) or not k_per_sample.is_contiguous():
            raise L.LnxError("predict_topk: k_per_sample must be contiguous int32 [B]")
        a.k_per_sample = _p(k_per_sample)
    if out is None:
        out = (torch.empty(a.B, T, a.K, dtype=torch.int64, device=dev), torch.empty(a.B, T, a.K, dtype=torch.float32, device=dev),
               torch.empty(a.B, T, dtype=torch.int32, device=dev), torch.empty(a.B, T, dtype=torch.int32, device=dev))
    for o, dt, shape in zip(out, (torch.int64, torch.float32, torch.int32, torch.int32), ((a.B, T, a.K), (a.B, T, a.K), (a.B, T), (a.B, T))):
        if o.dtype != dt or tuple(o.shape) != shape or not o.is_contiguous():
            raise L.LnxError(f"predict_topk: outputs must be contiguous int64 / fp32 [B, T, K] and int32 [B, T] x 2, got {tuple(o.shape)} {o.dtype}")
    a.ids, a.probs, a.count, a.flags = (_p(o) for o in out)
    L.check(L.lib().lnx_predict(C.byref(a), _stream()), "lnx_predict")
    return tuple(out)


def _hier_refine_rows(what, t, x, B, code, like=None):
    """[B, C] rows of one dtype with unit column stride -> the leading dimension (a padded view's stride(0))"""
    if x.dim() != 2 or x.shape[0] != B or code_of(x) != code or (x.shape[1] > 1 and x.stride(1) != 1):
        raise L.LnxError(f"{what}: level {t} must be [B, C] rows of one dtype (fp32 / bf16) with unit column stride, got {tuple(x.shape)} {x.dtype} strides {x.stride()}")
    if like is not None and x.shape[1] != like.shape[1]:
        raise L.LnxError(f"{what}: level {t} has {x.shape[1]} columns, expected {like.shape[1]}")
    return x.stride(0) if B > 1 else x.shape[1]


def _hier_refine_levels(what, a, rows, tables, modes, temps, noises):
    """The per-level fields both directions share: C, the tables, mode, temperature, noise (rows: per level a [B, C] tensor)."""
    T = len(rows)
    if not 1 <= T <= L.METRICS_MAX_TASKS or not (len(tables) == len(modes) == len(temps) == len(noises) == T):
        raise L.LnxError(f"{what}: {T} levels (1..{L.METRICS_MAX_TASKS}) need {T} tables / modes / temperatures / noise entries")
    a.dtype, a.B, a.n_tasks = code_of(rows[0]), rows[0].shape[0], T
    for t in range(T):
        k, Ct = a.level[t], rows[t].shape[1]
        k.C, k.mode, k.temperature = Ct, int(modes[t]), float(temps[t])
        if tables[t] is None or t == T - 1:
            continue
        Cp = rows[t + 1].shape[1]
        par, start, idx = tables[t]
        for name, tab, n in (("parent", par, Ct), ("child_start", start, Cp + 1), ("child_idx", idx, Ct)):
            if tab is not None and (tab.dtype != torch.int32 or tab.shape != (n,) or not tab.is_contiguous()):
                raise L.LnxError(f"{what}: level {t} {name} table must be contiguous int32 [{n}]")
        k.parent, k.child_start, k.child_idx = _p(par), _p(start), _p(idx)
        g = noises[t]
        if g is not None:
            if g.dtype != torch.float32 or g.shape != (a.B, Cp) or not g.is_contiguous():
                raise L.LnxError(f"{what}: level {t} noise must be contiguous fp32 [{a.B}, {Cp}]")
            k.noise = _p(g)


def hier_refine_fwd(bases, tables, modes, temps, noises, outs=None):
    """One lnx_hier_refine_fwd launch: out[t] = base[t] + log(prob[parent] + 1e-10) for every level, finest first (include/lnx.h).
    bases: per level [B, C] rows of one dtype (fp32 / bf16), unit column stride (padded views welcome); tables: per level
    (parent, child_start, child_idx) int32 device tensors or None (= pass-through; the coarsest level's entry is not read); modes / temps:
    per level L.HIER_ROUTE_* and the temperature; noises: per level fp32 [B, C_parent] or None.  outs: tensors laid out like the bases to
    write into (default: new ones; the coarsest level's is its base, which is not copied).  Returns (outs, stats [B, T, 2]); never synchronises."""
    a = L.HierRefineArgs()
    _hier_refine_levels("hier_refine_fwd", a, bases, tables, modes, temps, noises)
    T, B = a.n_tasks, a.B
    if outs is None:
        outs = [torch.empty_strided(x.shape, (x.stride(0) if B > 1 else x.shape[1], 1), dtype=x.dtype, device=x.device) for x in bases[:-1]] + [bases[-1]]
    for t in range(T):
        k = a.level[t]
        k.ld = _hier_refine_rows("hier_refine_fwd", t, bases[t], B, a.dtype)
        if _hier_refine_rows("hier_refine_fwd", t, outs[t], B, a.dtype, like=bases[t]) != k.ld:
            raise L.LnxError(f"hier_refine_fwd: level {t} out must have the leading dimension of its base ({k.ld})")
        k.base, k.out = _p(bases[t]), _p(outs[t])
    stats = torch.empty(B, T, 2, dtype=torch.float32, device=bases[0].device)
    a.stats = _p(stats)
    L.check(L.lib().lnx_hier_refine_fwd(C.byref(a), _stream()), "lnx_hier_refine_fwd")
    return list(outs), stats


def hier_refine_bwd(outs, stats, douts, tables, modes, temps, noises, dbases=None):
    """One lnx_hier_refine_bwd launch: the gradients of every level's base logits from the gradients of the refined ones.  outs / stats /
    noises: what hier_refine_fwd returned / was given; douts: per level [B, C] of the outs' dtype or None (= zeros); dbases: tensors to
    write into (default: new contiguous ones).  Returns dbases; never synchronises."""
    a = L.HierRefineArgs()
    _hier_refine_levels("hier_refine_bwd", a, outs, tables, modes, temps, noises)
    T, B = a.n_tasks, a.B
    if len(douts) != T:
        raise L.LnxError(f"hier_refine_bwd: {T} levels need {T} dout entries (None = zeros)")
    if stats.dtype != torch.float32 or stats.shape != (B, T, 2) or not stats.is_contiguous():
        raise L.LnxError(f"hier_refine_bwd: stats must be contiguous fp32 [{B}, {T}, 2]")
    if dbases is None:  # contiguous, and so are the douts beside them (one leading dimension per level)
        douts = [None if g is None else g.contiguous() for g in douts]
        dbases = [torch.empty(x.shape, dtype=x.dtype, device=x.device) for x in outs]
    for t in range(T):
        k = a.level[t]
        k.ld = _hier_refine_rows("hier_refine_bwd", t, outs[t], B, a.dtype)
        k.ldd = _hier_refine_rows("hier_refine_bwd", t, dbases[t], B, a.dtype, like=outs[t])
        if douts[t] is not None and _hier_refine_rows("hier_refine_bwd", t, douts[t], B, a.dtype, like=outs[t]) != k.ldd:
            raise L.LnxError(f"hier_refine_bwd: level {t} dout and dbase must share one leading dimension")
        k.out, k.dout, k.dbase = _p(outs[t]), _p(douts[t]), _p(dbases[t])
    a.stats = _p(stats)
    L.check(L.lib().lnx_hier_refine_bwd(C.byref(a), _stream()), "lnx_hier_refine_bwd")
    return list(dbases)


def preprocess_images(blob, blob_bytes, images, images_off, n, H, W, filter_code, mean, std, scratch, out):
    """lnx_preprocess on a batch that is already on the device: blob uint8 (descriptor table at images_off, tables, packed [h, w, 3]
    sources: include/lnx.h), images the HOST copy of the descriptor table (a ctypes array of L.PreprocessImage that
    lnx_preprocess_scratch_bytes has completed), scratch uint8 or None, out fp32 [n, 3, H, W] contiguous.  At most two launches, never
    synchronises."""
    if out.dtype != torch.float32 or tuple(out.shape) != (n, 3, H, W) or not out.is_contiguous():
        raise L.LnxError(f"preprocess_images: out must be contiguous fp32 [{n}, 3, {H}, {W}], got {tuple(out.shape)} {out.dtype}")
    if blob.dtype != torch.uint8 or (scratch is not None and scratch.dtype != torch.uint8):
        raise L.LnxError("preprocess_images: blob and scratch are uint8 buffers")
    a = L.PreprocessArgs()
    a.n, a.H, a.W, a.filter = int(n), int(H), int(W), int(filter_code)
    a.images = C.cast(images, C.POINTER(L.PreprocessImage))
    a.blob, a.blob_bytes, a.images_off = _p(blob), int(blob_bytes), int(images_off)
    a.scratch, a.scratch_bytes = _p(scratch), (0 if scratch is None else scratch.numel())
    a.mean[:] = [float(v) for v in mean]
    a.std[:] = [float(v) for v in std]
    a.out = _p(out)
    L.check(L.lib().lnx_preprocess(C.byref(a), _stream()), "lnx_preprocess")
    return out
