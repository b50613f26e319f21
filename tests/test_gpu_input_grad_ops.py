"""The input-gradient kernels through the C ABI (ops.stem_dgrad, ops.col2im_stem + ops.gemm_nt as the fallback composition,
ops.meta_input_grad) against the fp64 references of tests/input_grad_ref.py.

Exact probes: small-integer operands (exact in bf16, and exact in fp32 in ANY summation order at these sizes: |sum| <= 256 * 12 for the
stem, <= 1536 * 12 for the metadata) and a weight without symmetry, so a swapped row / column / tap cannot pass; compared with
torch.equal.  Random data: the bound of the project's fp32 NT-GEMM tests (tests/test_gpu_gemm.py: rtol 2e-5, atol 8e-5 against fp64 on
the operands as stored), which holds for bf16 operands too since the reference is formed from the rounded operands and both accumulate
in fp32."""
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests.input_grad_ref import asymmetric_weight, col2im_ref, integer_probe, meta_input_grad_ref, stem_dgrad_ref

pytestmark = pytest.mark.gpu
DT = {L.F32: torch.float32, L.BF16: torch.bfloat16}
SHAPES = [(4, 4), (8, 8), (12, 20), (32, 36), (64, 64)]  # one patch, less than a tile, non-square, tile seams inside and across rows
GUARD = 64  # floats of NaN either side of dx (256 bytes: dx stays 16-byte aligned)
NT_TOL = dict(rtol=2e-5, atol=8e-5)


def _guarded(B, Cin, H, W):
    n = B * Cin * H * W
    flat = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    return flat, flat[GUARD: GUARD + n].view(B, Cin, H, W)


def _check_guards(flat):
    assert torch.isnan(flat[:GUARD]).all() and torch.isnan(flat[-GUARD:]).all(), "a store outside dx"


def _dy(M, Cout, pad, dt, seed, random=False):
    """[M, Cout + pad] with NaN in the padding columns; the first Cout columns are the operand"""
    buf = torch.full((M, Cout + pad), float("nan"))
    buf[:, :Cout] = torch.randn(M, Cout, generator=torch.Generator().manual_seed(seed)) if random else integer_probe((M, Cout), -3, 3, seed)
    return buf.to(dt).cuda()


@pytest.mark.parametrize("dtype", [L.BF16, L.F32])
@pytest.mark.parametrize("Cin", [1, 3, 4])
@pytest.mark.parametrize("Cout", [96, 128, 192, 256])
def test_stem_dgrad_exact(Cout, Cin, dtype):
    assert ops.stem_dgrad_ok(dtype, Cin, 8, 8, Cout)
    w = asymmetric_weight(Cout, Cin, seed=Cout + Cin)
    wd = w.to(DT[dtype]).cuda()
    for H, W in SHAPES:
        for B in (1, 2, 3):
            M = B * (H // 4) * (W // 4)
            for pad in (0, 8):  # ldy == Cout, and ldy > Cout with NaN behind the row
                dy = _dy(M, Cout, pad, DT[dtype], seed=H * 100 + W * 10 + B)
                flat, dx = _guarded(B, Cin, H, W)
                ops.stem_dgrad(dy, wd, dx, Cout=Cout)
                ref = stem_dgrad_ref(dy.float().cpu(), w, B, Cin, H, W)
                assert torch.equal(dx.cpu().double(), ref), (H, W, B, pad)
                _check_guards(flat)


@pytest.mark.parametrize("dtype", [L.BF16, L.F32])
@pytest.mark.parametrize("Cin", [1, 3, 4])
@pytest.mark.parametrize("Cout", [32, 64])
def test_fallback_composition_exact(Cout, Cin, dtype):
    """lnx_gemm_nt on the transposed weight copy [Cin * 16, Cout], then lnx_col2im_stem: what the plan runs where lnx_stem_dgrad_ok says no"""
    assert not ops.stem_dgrad_ok(dtype, Cin, 8, 8, Cout)
    w = asymmetric_weight(Cout, Cin, seed=Cout + Cin)
    wt = w[:, : Cin * 16].t().contiguous().to(DT[dtype]).cuda()  # [Cin * 16, Cout]
    for H, W in SHAPES:
        for B in (1, 2, 3):
            M = B * (H // 4) * (W // 4)
            dy = _dy(M, Cout, 0, DT[dtype], seed=H * 100 + W * 10 + B)
            dcol = torch.full((M, Cin * 16), float("nan"), device="cuda")  # fp32 out of the GEMM, as the plan asks for it
            ops.gemm_nt(dy, wt, dcol)
            flat, dx = _guarded(B, Cin, H, W)
            ops.col2im_stem(dcol, dx)
            ref = stem_dgrad_ref(dy.float().cpu(), w, B, Cin, H, W)
            assert torch.equal(dx.cpu().double(), ref), (H, W, B)
            _check_guards(flat)


@pytest.mark.parametrize("dtype", [L.BF16, L.F32])
def test_col2im_inverts_im2col(dtype):
    """col2im(im2col(x)) == x (as stored), with a padded patch row (ldp = 64 > Cin * 16) whose padding is never read"""
    for Cin in (1, 3, 4):
        B, H, W = 2, 12, 20
        x = integer_probe((B, Cin, H, W), -100, 100, seed=Cin).cuda()
        patches = torch.empty(B * 3 * 5, 64, device="cuda", dtype=DT[dtype])
        ops.im2col_stem(x, patches)
        assert torch.equal(col2im_ref(patches.float(), B, Cin, H, W), x.cpu().double())
        patches[:, Cin * 16:] = float("nan")
        flat, dx = _guarded(B, Cin, H, W)
        ops.col2im_stem(patches, dx)
        assert torch.equal(dx, x)
        _check_guards(flat)


@pytest.mark.parametrize("dtype", [L.BF16, L.F32])
@pytest.mark.parametrize("Cout", [32, 96, 128, 192, 256])
def test_stem_dgrad_random_within_the_nt_gemm_bound(Cout, dtype):
    B, Cin, H, W = 3, 3, 32, 36
    M = B * (H // 4) * (W // 4)
    gen = torch.Generator().manual_seed(Cout)
    w = torch.zeros(Cout, 64)
    w[:, : Cin * 16] = torch.randn(Cout, Cin * 16, generator=gen) * 0.25
    wd = w.to(DT[dtype]).cuda()
    dy = _dy(M, Cout, 8, DT[dtype], seed=Cout + 1, random=True)
    flat, dx = _guarded(B, Cin, H, W)
    if ops.stem_dgrad_ok(dtype, Cin, H, W, Cout):
        ops.stem_dgrad(dy, wd, dx, Cout=Cout)
    else:
        dcol = torch.empty(M, Cin * 16, device="cuda")
        ops.gemm_nt(dy, wd[:, : Cin * 16].t().contiguous(), dcol, K=Cout)
        ops.col2im_stem(dcol, dx)
    ref = stem_dgrad_ref(dy.float().cpu(), wd.float().cpu(), B, Cin, H, W)
    err = (dx.cpu().double() - ref).abs().max().item()
    print(f"[stem dgrad Cout={Cout} {DT[dtype]}] max abs error {err:.3e} at |ref| max {ref.abs().max().item():.2f}")
    torch.testing.assert_close(dx.cpu().double(), ref, **NT_TOL)
    _check_guards(flat)


def _meta_case(B, Cc, dim, seed, random=False):
    gen = torch.Generator().manual_seed(seed)
    if random:
        dp0, w0 = torch.randn(B, Cc, generator=gen), torch.randn(Cc, 16, generator=gen)
    else:
        dp0, w0 = integer_probe((B, Cc), -3, 3, seed), integer_probe((Cc, 16), -4, 4, seed + 1)
    w0[:, dim:] = float("nan")  # the arena pads with zeros; whatever is there must not be read into a sum
    return dp0.cuda(), w0.cuda()


@pytest.mark.parametrize("dim", [1, 2, 3, 10, 16])
@pytest.mark.parametrize("Cc", [128, 384, 768, 1024, 1536])
def test_meta_input_grad_exact(Cc, dim):
    off, width = 1, dim + 3
    for B in (1, 15, 16, 17, 33):
        dp0, w0 = _meta_case(B, Cc, dim, seed=Cc + dim + B)
        for accumulate in (False, True):
            base = integer_probe((B, width), -50, 50, seed=B).cuda()
            dmeta = base.clone()
            if not accumulate:
                dmeta[:, off: off + dim] = float("nan")  # the write form reads nothing of what it overwrites
            ops.meta_input_grad([(dp0, w0, dim, off)], dmeta, accumulate=accumulate)
            ref = meta_input_grad_ref([(dp0, w0, dim, off)], B, width, base=base if accumulate else None)
            if not accumulate:  # the columns no head covers keep what they held
                ref[:, :off] = base[:, :off].double().cpu()
                ref[:, off + dim:] = base[:, off + dim:].double().cpu()
            assert torch.equal(dmeta.cpu().double(), ref), (B, accumulate)
            again = base.clone()
            ops.meta_input_grad([(dp0, w0, dim, off)], again, accumulate=accumulate)
            assert torch.equal(again, dmeta)


def test_meta_input_grad_many_heads_random_and_bitwise_repeatable():
    """LNX_MAX_META heads of mixed widths in one launch (write), then a second launch that adds (the two RoPE stages of a model); random
    data inside the fp32 bound, and the same bits from a second run."""
    B = 33
    dims = [1, 2, 3, 10, 16, 4, 7, 5]
    widths = [128, 384, 768, 1024, 1536, 256, 512, 2048]
    offs = [sum(dims[:i]) for i in range(len(dims))]
    width = sum(dims)
    stage4 = [(*_meta_case(B, c, d, seed=i, random=True), d, o) for i, (c, d, o) in enumerate(zip(widths, dims, offs))]
    stage3 = [(*_meta_case(B, c // 2, d, seed=100 + i, random=True), d, o) for i, (c, d, o) in enumerate(zip(widths, dims, offs))]
    runs = []
    for _ in range(2):
        dmeta = torch.full((B, width), float("nan"), device="cuda")
        ops.meta_input_grad(stage4, dmeta, accumulate=False)
        ops.meta_input_grad(stage3, dmeta, accumulate=True)
        runs.append(dmeta)
    assert torch.equal(runs[0], runs[1])
    ref = meta_input_grad_ref(stage4 + stage3, B, width)
    err = (runs[0].cpu().double() - ref).abs().max().item()
    print(f"[meta input grad] max abs error {err:.3e} at |ref| max {ref.abs().max().item():.1f}")
    torch.testing.assert_close(runs[0].cpu().double(), ref, **NT_TOL)
