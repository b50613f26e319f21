"""csrc/gemm_fp8.hip at every K-loop length, tile seam and epilogue form: the 256x128-tile gemm_nt_fp8_kernel (per-tensor scales and
MXFP8), the 256x256-tile gemm_nt_mx8_kernel, their MXFP8-copy epilogues, and the amax / quantize_fp8 / quantize_mxfp8 streaming kernels.

Method.  Every call goes through the C ABI (linnaeus_amd.ops); lnx_last_nt_kernel says which GEMM kernel ran and every case asserts it.
  * Exact probes (tests/fp8_ref.py: probe_operands): operand BYTES and scales written directly, one operand with a single non-zero per
    row, so each output is one product a 2^ea w 2^ew -- a bf16 value -- and the comparison is torch.equal.  A wrong scale byte, chunk
    order, stage, row clamp or row permutation moves a power of two or picks another element: nothing hides inside a tolerance, and
    nothing in the expected value comes from the code under test.
  * Dense data through the project's quantisers against the fp64 product of the dequantised operands, every form nt_fp8_carries lists,
    at the project's own tolerances (test_gpu_ops.py: test_mxfp8_quantize_and_gemm, test_mxfp8_256x256_kernel_at_xl_rows).
  * Every output is a window of a larger NaN-filled allocation (guard rows above and below, guard columns left and right, so every
    row pitch is wider than the row); everything outside the window must still be NaN after the call (uint8: a sentinel byte that
    no quantiser emits).  Operands with a pitch are windows of wider tensors whose surroundings are NaN (bytes: 0x7f, e4m3fn's NaN).
  * Quantisers: byte for byte against fp8_ref, past both grid caps, from strided rows, with a caller's amax below the data's maximum.
"""
import ctypes as C

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests import fp8_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GR, GC = 8, 8                 # guard rows / guard columns (elements) round a float window; 8 bf16 = 16 bytes, 8 fp32 = 32 bytes
GC8 = 16                      # guard columns round a byte window
SENT8, SENT_SC = 0x7F, 0xFF   # e4m3fn NaN / E8M0 NaN: the clamps in front of the conversions never produce either


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _last_kernel():
    return L.lib().lnx_last_nt_kernel()


class Window:
    """An [M, N] window of a larger buffer filled with NaN (floats) or a sentinel byte (uint8)."""

    def __init__(self, M, N, dtype):
        self.M, self.N = M, N
        self.gc = GC8 if dtype == torch.uint8 else GC
        self.fill = SENT8 if dtype == torch.uint8 else NAN
        self.buf = torch.full((M + 2 * GR, N + 2 * self.gc), self.fill, device="cuda", dtype=dtype)
        self.t = self.buf[GR:GR + M, self.gc:self.gc + N]
        assert self.t.stride(0) > N and self.t.data_ptr() % 16 == 0

    def assert_guards(self, what):
        g = self.buf.clone()
        g[GR:GR + self.M, self.gc:self.gc + self.N] = self.fill
        bad = ~g.isnan() if g.is_floating_point() else g != self.fill
        if bad.any():
            r, c = [int(v) for v in bad.nonzero()[0]]
            raise AssertionError(f"{what}: {int(bad.sum())} elements outside the [{self.M}, {self.N}] window were written, first at "
                                 f"row {r - GR}, column {c - self.gc} (relative to the window)")


def _scale_window(N, M):
    """c8_scales [N/128, M, 4] inside a sentinel-filled flat buffer."""
    n = (N // 128) * M * 4
    flat = torch.full((n + 32,), SENT_SC, device="cuda", dtype=torch.uint8)
    return flat, flat[16:16 + n].view(N // 128, M, 4)


def _assert_scale_guards(flat, what):
    assert (flat[:16] == SENT_SC).all() and (flat[-16:] == SENT_SC).all(), f"{what}: bytes round the scale array were written"


def _widen(t):
    """The same values as a window (pitch > row) of a wider tensor whose other columns are NaN / 0x7f."""
    rows, cols = t.shape
    gc = GC8 if t.dtype == torch.uint8 else GC
    wide = torch.full((rows, cols + 2 * gc), SENT8 if t.dtype == torch.uint8 else NAN, device=t.device, dtype=t.dtype)
    wide[:, gc:gc + cols] = t
    v = wide[:, gc:gc + cols]
    assert v.stride(0) > cols and v.data_ptr() % 16 == 0
    return v


def _assert_exact(out, expected, side, K, what):
    if torch.equal(out, expected):
        return
    bad = out != expected
    bad |= out.isnan()
    m, n = [int(v) for v in bad.nonzero()[0]]
    k = int(R.probe_positions(max(out.shape), K)[m if side == "A" else n])
    raise AssertionError(f"{what}: {int(bad.sum())} of {out.numel()} outputs differ; first at (m, n) = ({m}, {n}), probed k = {k} "
                         f"(K slice {k // 128}, block {k // 32 % 4}): got {out[m, n].item()!r}, expected {expected[m, n].item()!r}; "
                         f"rows with a difference: {int(bad.any(1).sum())}, columns: {int(bad.any(0).sum())}")


def _probe(M, N, K, side, scales, seed, kernel, wide=False):
    p = R.probe_operands(M, N, K, side, seed, scales=scales, device="cuda")
    A8, W8 = (_widen(p["A8"]), _widen(p["W8"])) if wide else (p["A8"], p["W8"])
    w = Window(M, N, torch.bfloat16)
    if scales == "mx":
        ops.gemm_nt_mxfp8(A8, p["sa"], W8, p["sw"], w.t)
    else:
        ops.gemm_nt_fp8(A8, p["sa"], W8, p["sw"], w.t)
    assert _last_kernel() == kernel
    what = f"probe M={M} N={N} K={K} side={side} scales={scales}"
    w.assert_guards(what)
    _assert_exact(w.t, p["expected"], side, K, what)


# ------------------------------------------------------------------------------------------------------------------------------------
# B. exact probes
# ------------------------------------------------------------------------------------------------------------------------------------
K_SWEEP = [256, 384, 512, 640, 896, 1152, 1536]   # nk = K / 128 = 2, 3, 4, 5, 7, 9, 12: both parities, every residue mod 3 (the ring)


@pytest.mark.parametrize("side", ["A", "W"])
@pytest.mark.parametrize("scales", ["mx", "pow2"])
@pytest.mark.parametrize("K", K_SWEEP)
def test_256x128_probe_k_sweep(K, scales, side):
    """gemm_nt_fp8_kernel, plain form, at every K-loop length class.  Side A: 1537 rows (at least K rows, so every k position and every
    block-scale byte of A is probed, plus a one-row last tile) x 208 columns; side W: max(K, 256) + 16 columns, every k of W probed."""
    M, N = (1536 + 1, 208) if side == "A" else (257, max(K, 256) + 16)
    _probe(M, N, K, side, scales, seed=K + (side == "W"), kernel=L.NT_KERNEL_FP8, wide=K in (384, 1152))


@pytest.mark.parametrize("side", ["A", "W"])
def test_256x128_probe_arbitrary_per_tensor_scales(side):
    """Per-tensor scales that are no powers of two: the expected value restates the kernel's two roundings, (fp32 accumulator) *
    fp32(sa * sw), then bf16."""
    M, N = (641, 208) if side == "A" else (257, 656)
    _probe(M, N, 640, side, "arbitrary", seed=3, kernel=L.NT_KERNEL_FP8)


@pytest.mark.parametrize("N", [16, 64, 80, 128, 144, 208, 272])
@pytest.mark.parametrize("M", [256, 257, 449, 513])
def test_256x128_probe_tile_seams(M, N):
    """K = 384 (nk = 3) at the smallest sizes that put a seam on the 256-row tile, the 64-row wave tile, the 128-column tile and the
    64-column wave half; N = 16 makes almost every W row and W scale fetch a clamped one."""
    for scales in ("mx", "pow2"):
        for side in ("A", "W"):
            _probe(M, N, 384, side, scales, seed=M * 1000 + N, kernel=L.NT_KERNEL_FP8)


@pytest.mark.parametrize("side", ["A", "W"])
def test_256x128_probe_at_a_256x256_shape_with_the_switch_off(side, monkeypatch):
    """LNX_FP8_X8=0 (read on every call) sends a product the 256x256 kernel would take to the 256x128 MX kernel: 128 row tiles x 2."""
    monkeypatch.setenv("LNX_FP8_X8", "0")
    _probe(32513, 256, 384, side, "mx", seed=17, kernel=L.NT_KERNEL_FP8)
    monkeypatch.delenv("LNX_FP8_X8")
    _probe(32513, 256, 384, side, "mx", seed=17, kernel=L.NT_KERNEL_MX8)


@pytest.mark.parametrize("side", ["A", "W"])
@pytest.mark.parametrize("K", [256, 384, 640])                                    # nk = K / 64 = 4 (the shortest loop), 6, 10
@pytest.mark.parametrize("M,N", [(32513, 256), (32768, 256), (16385, 512)])       # >= 128 tiles; one-row last tile / none
def test_256x256_probe(M, N, K, side):
    """gemm_nt_mx8_kernel.  Side W at N = 256 probes all 256 rows of the W tile, permuted row order included; side A every A row's
    scale byte selection (sb = 2 (kt & 1)) at every k."""
    _probe(M, N, K, side, "mx", seed=M + N + K, kernel=L.NT_KERNEL_MX8, wide=(K == 384))


# ------------------------------------------------------------------------------------------------------------------------------------
# C. dense data, every carried form
# ------------------------------------------------------------------------------------------------------------------------------------
def _dense_operands(M, N, K, kind, seed, wide):
    """Activations with per-block factors 2^-4 .. 2^4 and weights / sqrt(K), as test_mxfp8_quantize_and_gemm scales them, through the
    project's quantisers; the reference is the fp64 product of what the bytes and scales stand for (dequantised by fp8_ref)."""
    gen = _gen(seed)
    a = (torch.randn(M, K, device="cuda", generator=gen)
         * torch.exp2(torch.randint(-4, 5, (M, K // 32, 1), device="cuda", generator=gen).float()).expand(M, K // 32, 32).reshape(M, K)).bfloat16()
    w = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).bfloat16()
    if kind == "mx":
        a8, sa = ops.quantize_mxfp8(a)
        w8, sw = ops.quantize_mxfp8(w)
        ad = (R.e4m3_to_float(a8.view(torch.uint8)).double().view(M, K // 32, 32) * torch.exp2(R.unpack_scales(sa).double() - 127).unsqueeze(-1)).view(M, K)
        wd = (R.e4m3_to_float(w8.view(torch.uint8)).double().view(N, K // 32, 32) * torch.exp2(R.unpack_scales(sw).double() - 127).unsqueeze(-1)).view(N, K)
    else:
        a8, sa = ops.quantize_fp8(a)
        w8, sw = ops.quantize_fp8(w)
        ad = R.e4m3_to_float(a8.view(torch.uint8)).double() * sa.double()
        wd = R.e4m3_to_float(w8.view(torch.uint8)).double() * sw.double()
    ref = ad @ wd.t()
    a8, w8 = a8.view(torch.uint8), w8.view(torch.uint8)
    if wide:
        a8, w8 = _widen(a8), _widen(w8)
    return a8, sa, w8, sw, ref, gen


def _gelu_grad(aux):
    xa = aux.double().requires_grad_(True)
    torch.nn.functional.gelu(xa).sum().backward()
    return xa.grad


def _all_forms(M, N, K, kind, seed, kernel, wide):
    a8, sa, w8, sw, ref, gen = _dense_operands(M, N, K, kind, seed, wide)
    mx = kind == "mx"

    def run(out, **kw):
        if mx:
            ops.gemm_nt_mxfp8(a8, sa, w8, sw, out, **kw)
        else:
            ops.gemm_nt_fp8(a8, sa, w8, sw, out, **kw)
        assert _last_kernel() == kernel

    tag = f"{kind} M={M} N={N} K={K}"
    tol = 8e-3 * max(1.0, ref.abs().max().item())
    bias = torch.randn(N, device="cuda", generator=gen)
    h = ref + bias.double()
    # plain
    o = Window(M, N, torch.bfloat16)
    run(o.t)
    o.assert_guards(f"{tag} plain")
    torch.testing.assert_close(o.t.double(), ref, rtol=8e-3, atol=tol)
    # bias
    o = Window(M, N, torch.bfloat16)
    run(o.t, bias=bias)
    o.assert_guards(f"{tag} bias")
    torch.testing.assert_close(o.t.double(), h, rtol=8e-3, atol=tol)
    # bias + GELU + pre-activation copy
    o, pre = Window(M, N, torch.bfloat16), Window(M, N, torch.bfloat16)
    run(o.t, bias=bias, act=L.ACT_GELU, c2=pre.t)
    o.assert_guards(f"{tag} gelu out")
    pre.assert_guards(f"{tag} gelu c2")
    torch.testing.assert_close(pre.t.double(), h, rtol=8e-3, atol=tol)
    torch.testing.assert_close(o.t.double(), torch.nn.functional.gelu(h), rtol=8e-3, atol=tol)
    # GELU_BWD: x GELU'(aux), aux with a pitch of its own
    aux = _widen(torch.randn(M, N, device="cuda", generator=gen).bfloat16())
    ob = Window(M, N, torch.bfloat16)
    run(ob.t, act=L.ACT_GELU_BWD, aux=aux)
    ob.assert_guards(f"{tag} gelu_bwd")
    torch.testing.assert_close(ob.t.double(), ref * _gelu_grad(aux), rtol=1e-2, atol=1.25 * tol)
    if mx and N % 128 == 0:
        # the same two forms with the MXFP8 copy of the output: the bf16 outputs do not change, and the copy is what quantising them gives
        for name, first, kw in (("gelu + c8", o, dict(bias=bias, act=L.ACT_GELU)), ("gelu_bwd + c8", ob, dict(act=L.ACT_GELU_BWD, aux=aux))):
            o2, pre2, c8 = Window(M, N, torch.bfloat16), Window(M, N, torch.bfloat16), Window(M, N, torch.uint8)
            flat, c8s = _scale_window(N, M)
            if "bias" in kw:
                kw["c2"] = pre2.t
            run(o2.t, c8=c8.t, c8_scales=c8s, **kw)
            o2.assert_guards(f"{tag} {name} out")
            c8.assert_guards(f"{tag} {name} c8")
            _assert_scale_guards(flat, f"{tag} {name}")
            assert torch.equal(o2.t, first.t), f"{tag} {name}: the bf16 output differs from the form without c8"
            if "bias" in kw:
                pre2.assert_guards(f"{tag} {name} c2")
                assert torch.equal(pre2.t, pre.t)
            r8, rsc = ops.quantize_mxfp8(o2.t.contiguous())
            assert torch.equal(c8s, rsc), f"{tag} {name}: block scales"
            assert torch.equal(c8.t, r8.view(torch.uint8)), f"{tag} {name}: bytes"
            q, e = R.mx_reference(o2.t.contiguous())
            assert torch.equal(c8.t, q.view(torch.uint8)) and torch.equal(R.unpack_scales(c8s), e)
    # fp32 output: bias + residual + DropPath row scale.  37 rows per sample: the kernels' per-row division, a sample boundary inside every
    # tile and off the 64- / 32-row wave-tile seams; 100: the two-samples-per-64-rows shortcut of the 256x128 epilogue (>= 64)
    res = _widen(torch.randn(M, N, device="cuda", generator=gen))
    for rps in (37, 100):
        ns = (M + rps - 1) // rps
        rs = (torch.rand(ns, device="cuda", generator=gen) > 0.2).float() / 0.8 + torch.rand(ns, device="cuda", generator=gen) * 0.25
        o32 = Window(M, N, torch.float32)
        run(o32.t, bias=bias, res=res, rowscale=rs, rows_per_sample=rps)
        o32.assert_guards(f"{tag} fp32 rps={rps}")
        rowf = rs.double().repeat_interleave(rps)[:M, None]
        torch.testing.assert_close(o32.t.double(), res.double() + rowf * h, rtol=1e-4, atol=1e-4 * max(1.0, ref.abs().max().item()))


DENSE_256x128 = [(513, 208, 384), (449, 144, 640), (257, 384, 1152), (513, 384, 384)]   # (the last one: N % 128 == 0, the c8 forms)


@pytest.mark.parametrize("kind", ["mx", "pt"])
@pytest.mark.parametrize("M,N,K", DENSE_256x128)
def test_256x128_dense_every_form(M, N, K, kind):
    _all_forms(M, N, K, kind, seed=M + N + K, kernel=L.NT_KERNEL_FP8, wide=(K == 640))


@pytest.mark.parametrize("M,N,K", [(32513, 256, 256), (16385, 512, 384)])
def test_256x256_dense_every_form(M, N, K):
    _all_forms(M, N, K, "mx", seed=M + N + K, kernel=L.NT_KERNEL_MX8, wide=(K == 384))


def test_256x128_dense_every_form_with_the_switch_off(monkeypatch):
    """The default fp8 backward's dH hand-over (GELU_BWD + c8) and the other forms on the 256x128 MX kernel at a 256x256 shape."""
    monkeypatch.setenv("LNX_FP8_X8", "0")
    _all_forms(32513, 256, 256, "mx", seed=5, kernel=L.NT_KERNEL_FP8, wide=False)


# ---- refusals: host side, nothing launches ----
def _refusal_args(M, N, K, mx):
    A8 = torch.full((M, K), 0x38, device="cuda", dtype=torch.uint8)
    W8 = torch.full((N, K), 0x38, device="cuda", dtype=torch.uint8)
    if mx:
        sa = torch.full((K // 128, M, 4), 127, device="cuda", dtype=torch.uint8)
        sw = torch.full((K // 128, N, 4), 127, device="cuda", dtype=torch.uint8)
    else:
        sa = sw = torch.ones(1, device="cuda")
    return A8, sa, W8, sw


def _refused(mx, A8, sa, W8, sw, out, **kw):
    before = L.lib().lnx_nt_kernel_launches(L.NT_KERNEL_FP8) + L.lib().lnx_nt_kernel_launches(L.NT_KERNEL_MX8)
    with pytest.raises(L.LnxError):
        (ops.gemm_nt_mxfp8 if mx else ops.gemm_nt_fp8)(A8, sa, W8, sw, out, **kw)
    torch.cuda.synchronize()
    assert L.lib().lnx_nt_kernel_launches(L.NT_KERNEL_FP8) + L.lib().lnx_nt_kernel_launches(L.NT_KERNEL_MX8) == before
    assert out.isnan().all()


@pytest.mark.parametrize("mx", [True, False])
@pytest.mark.parametrize("M,N,K", [(255, 128, 256), (512, 128, 128), (512, 128, 320)])
def test_refuses_shapes_the_kernels_cannot_run(M, N, K, mx):
    """M < 256 (a clamped row would be fetched for a whole tile), K = 128 (the pipeline's prologue issues two K slices), K % 128 != 0."""
    out = torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16)
    _refused(mx, *_refusal_args(M, N, K, mx), out)


@pytest.mark.parametrize("mx", [True, False])
@pytest.mark.parametrize("M,N,K", [(512, 128, 256), (32513, 256, 256)])
def test_refuses_forms_the_kernels_do_not_carry(M, N, K, mx):
    """An fp32 output without a residual, and bias + GELU without the pre-activation copy -- a form the bf16 dispatch carries and
    nt_fp8_carries does not: refused, never run as something else (the second shape is one the 256x256 kernel takes)."""
    args = _refusal_args(M, N, K, mx)
    bias = torch.zeros(N, device="cuda")
    _refused(mx, *args, torch.full((M, N), NAN, device="cuda", dtype=torch.float32))
    _refused(mx, *args, torch.full((M, N), NAN, device="cuda", dtype=torch.float32), bias=bias)
    _refused(mx, *args, torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16), bias=bias, act=L.ACT_GELU)


def test_refuses_bad_mxfp8_copies_and_misaligned_scales():
    M, K = 512, 256
    for N, kw in ((128, dict()),                                                    # c8 with the plain form
                  (128, dict(bias=True)),                                           # c8 with the bias form
                  (208, dict(bias=True, act=L.ACT_GELU, c2=True))):                 # c8 with N % 128 != 0
        A8, sa, W8, sw = _refusal_args(M, N, K, True)
        kw = dict(kw)
        if kw.get("bias"):
            kw["bias"] = torch.zeros(N, device="cuda")
        if kw.get("c2"):
            kw["c2"] = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
        c8 = torch.full((M, N), SENT8, device="cuda", dtype=torch.uint8)
        c8s = torch.full((2, M, 4), SENT_SC, device="cuda", dtype=torch.uint8)
        _refused(True, A8, sa, W8, sw, torch.full((M, N), NAN, device="cuda", dtype=torch.bfloat16), c8=c8, c8_scales=c8s, **kw)
        assert (c8 == SENT8).all() and (c8s == SENT_SC).all()
    # block-scale arrays one byte off their 4-byte alignment, either one
    A8, sa, W8, sw = _refusal_args(M, 128, K, True)

    def off_by_one(s):
        flat = torch.full((s.numel() + 4,), 127, device="cuda", dtype=torch.uint8)
        v = flat[1:1 + s.numel()].view(s.shape)
        assert v.data_ptr() % 4 == 1
        return v

    out = torch.full((M, 128), NAN, device="cuda", dtype=torch.bfloat16)
    _refused(True, A8, off_by_one(sa), W8, sw, out)
    _refused(True, A8, sa, W8, off_by_one(sw), out)


# ------------------------------------------------------------------------------------------------------------------------------------
# D. quantisers
# ------------------------------------------------------------------------------------------------------------------------------------
def _amax(x):
    am = torch.zeros(1, device="cuda", dtype=torch.float32)
    L.check(L.lib().lnx_amax(C.c_void_p(x.data_ptr()), ops.code_of(x), C.c_int64(x.stride(0)), x.shape[0], x.shape[1], C.c_void_p(am.data_ptr()),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_amax")
    return am


def _u8(t):
    return t.view(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_fp8_past_the_grid_cap(dtype):
    """4352 x 4096 = 17.8 M elements: quantize_fp8_kernel's 4096-block grid covers 16.8 M, amax_kernel's 2048 blocks 2.1 M (fp32) /
    4.2 M (bf16) per pass, so both grid-stride loops run.  The maximum sits, negative, in the last row: the last pass must see it."""
    rows, cols = 4352, 4096
    x = torch.randn(rows, cols, device="cuda", generator=_gen(rows)).to(dtype)
    x[rows - 1, cols - 5] = -9.25
    assert x.float().abs().max().item() == 9.25
    am = _amax(x)
    assert am.item() == 9.25
    x8, sx = ops.quantize_fp8(x)
    q, s = R.fp8_reference(x, 9.25)
    assert torch.equal(sx, s)
    assert torch.equal(_u8(x8), _u8(q))
    assert _u8(x8)[rows - 1, cols - 5] == 0xFE


def test_quantize_mxfp8_past_the_grid_cap():
    """16640 x 4096 = 68.2 M elements = 2.13 M blocks: quantize_mxfp8_kernel's 8192-block grid covers 2.10 M per pass."""
    rows, cols = 16640, 4096
    gen = _gen(rows)
    x = torch.randn(rows, cols, device="cuda", generator=gen)
    x = (x.view(rows, cols // 32, 32) * torch.exp2(torch.randint(-6, 7, (rows, cols // 32, 1), device="cuda", generator=gen).float())).view(rows, cols).bfloat16()
    x[rows - 1, cols - 5] = -3072.0
    assert _amax(x).item() == x.float().abs().max().item() == 3072.0
    x8, sx = ops.quantize_mxfp8(x)
    q, e = R.mx_reference(x)
    assert torch.equal(R.unpack_scales(sx), e)
    assert torch.equal(sx, R.pack_scales(e))
    assert torch.equal(_u8(x8), _u8(q))
    assert torch.equal(_u8(x8)[-64:], _u8(q)[-64:]) and torch.equal(R.unpack_scales(sx)[-64:], e[-64:])   # (the rows of the second pass)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantisers_read_strided_rows(dtype):
    """x = columns 128 .. 128 + cols of a wider tensor, as the plan quantises (rows of a concatenated buffer).  The columns on either
    side hold 1e30: one element read from outside the window changes amax, a block scale or a byte."""
    rows, cols = 301, 384
    wide = torch.full((rows, 128 + cols + 64), 1e30, device="cuda", dtype=dtype)
    wide[:, 128:128 + cols] = (torch.randn(rows, cols, device="cuda", generator=_gen(7)) * 3).to(dtype)
    x = wide[:, 128:128 + cols]
    xc = x.contiguous()
    assert x.stride(0) > cols and xc.stride(0) == cols
    assert _amax(x).item() == _amax(xc).item() == xc.float().abs().max().item()
    x8, sx = ops.quantize_fp8(x)
    c8, sc = ops.quantize_fp8(xc)
    q, s = R.fp8_reference(xc, xc.float().abs().max())
    assert torch.equal(sx, sc) and torch.equal(sx, s)
    assert torch.equal(_u8(x8), _u8(c8)) and torch.equal(_u8(x8), _u8(q))
    m8, ms = ops.quantize_mxfp8(x)
    n8, ns = ops.quantize_mxfp8(xc)
    q, e = R.mx_reference(xc)
    assert torch.equal(ms, ns) and torch.equal(R.unpack_scales(ms), e)
    assert torch.equal(_u8(m8), _u8(n8)) and torch.equal(_u8(m8), _u8(q))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_fp8_with_a_callers_amax_saturates(dtype):
    """Delayed scaling: amax = half the tensor's maximum.  Everything beyond +-amax must come out as +-448 (0x7e / 0xfe); 0x7f / 0xff are
    e4m3fn's NaN, which an unclamped conversion would produce."""
    x = (torch.randn(1000, 512, device="cuda", generator=_gen(11)) * 3).to(dtype)
    t = (x.float().abs().max() / 2).reshape(1)
    x8, sx = ops.quantize_fp8(x, amax=t)
    q, s = R.fp8_reference(x, t)
    assert torch.equal(sx, s) and sx.item() == torch.tensor(t.double().item() / 448.0, dtype=torch.float32).item()
    b = _u8(x8)
    assert torch.equal(b, _u8(q))
    over, under = x.float() > t, x.float() < -t
    assert over.sum() > 100 and under.sum() > 100
    assert (b[over] == 0x7E).all() and (b[under] == 0xFE).all()
    assert not ((b & 0x7F) == 0x7F).any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantize_fp8_of_zeros(dtype):
    x8, sx = ops.quantize_fp8(torch.zeros(64, 128, device="cuda", dtype=dtype))
    assert sx.item() == 1.0 and not _u8(x8).any()
