"""The fp64 restatement tests/dwconv_ref.py (the reference of tests/test_gpu_dwconv_walks.py) against the oracle's conv2d + autograd
at fp64 rounding, against the reference's recorded output, and its walk arithmetic on a case worked out by hand.  No GPU."""
import numpy as np
import pytest
import torch

from oracle import mformer_oracle as O
from tests.dwconv_ref import dwconv7_ref, mfma_fwd_walk, mfma_wgrad_walk, valu_fwd_walk, valu_wgrad_walk, walk_crossings


@pytest.mark.parametrize("B,H,W,C_", [(2, 1, 1, 3), (1, 2, 9, 5), (3, 5, 3, 2), (2, 7, 6, 4), (1, 13, 15, 3), (2, 9, 23, 7)])
@pytest.mark.parametrize("with_bias", [True, False])
def test_matches_oracle_and_autograd(B, H, W, C_, with_bias):
    gen = torch.Generator().manual_seed(B + 10 * H + 100 * W + C_)
    x = torch.randn(B, H, W, C_, generator=gen, dtype=torch.float64)
    w = torch.randn(C_, 1, 7, 7, generator=gen, dtype=torch.float64)
    bias = torch.randn(C_, generator=gen, dtype=torch.float64)
    dy = torch.randn(B, H, W, C_, generator=gen, dtype=torch.float64)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = bias.clone().requires_grad_(True)
    ref = O.depthwise_conv7(xr, wr, br if with_bias else torch.zeros_like(br))
    ref.backward(dy.permute(0, 3, 1, 2))
    y, dx, dw, db = dwconv7_ref(x, w, bias if with_bias else None, dy)
    tol = dict(rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(y, ref.detach().permute(0, 2, 3, 1), **tol)
    torch.testing.assert_close(dx, xr.grad.permute(0, 2, 3, 1), **tol)
    torch.testing.assert_close(dw, wr.grad.reshape(C_, 7, 7), **tol)
    torch.testing.assert_close(db, dy.sum((0, 1, 2)), **tol)
    # the data gradient is the same convolution with the taps turned by 180 degrees (how the kernels compute it: flip = 1)
    torch.testing.assert_close(dwconv7_ref(dy, w.reshape(C_, 49).flip(1))[0], dx, **tol)
    assert dwconv7_ref(x, w, bias)[1:] == (None, None, None)


def test_matches_recorded_reference_output(golden_dir):
    """cnb_dw: the reference's own ConvNeXt block's dwconv output (tests/golden/gen/make_golden.py), tolerance of test_oracle_golden.py"""
    z = np.load(f"{golden_dir}/per_op.npz")
    x = torch.from_numpy(z["cnb_x"])  # NCHW
    w = O.seeded_fill("stages.0.0.dwconv.weight", (8, 1, 7, 7), 20251003)
    b = O.seeded_fill("stages.0.0.dwconv.bias", (8,), 20251003)
    y = dwconv7_ref(x.permute(0, 2, 3, 1), w, b)[0].permute(0, 3, 1, 2)
    np.testing.assert_allclose(y.numpy(), z["cnb_dw"], rtol=1e-5, atol=1e-6)


def test_walk_arithmetic_by_hand():
    """the sm stage-0 shape at batch 24 on 256 compute units: 16 14x14 tiles per image, 384 tiles, 85 workgroups per channel block
    -> walks of 5 (77 of them, the last one 4 long), which cross tile rows and images"""
    f = mfma_fwd_walk(24, 56, 56, 96, 256)
    assert (f["ntile"], f["per"], f["chunks"]) == (384, 5, 77)
    assert walk_crossings(f["ntile"], f["per"], f["tiles_h"], f["tiles_w"]) == (True, True, True)
    assert mfma_fwd_walk(5, 14, 28, 128, 256)["per"] == 1 and mfma_fwd_walk(1, 56, 56, 32, 256)["per"] == 1
    g = mfma_wgrad_walk(64, 56, 56, 96, 256)  # 8 14x28 tiles per image, 85 walkers of 7 -> 74 walkers, 222 pairs in a grid of 16 * 28
    assert (g["ntile"], g["per"], g["walkers"], g["pairs"], g["grid"]) == (512, 7, 74, 222, 448)
    assert walk_crossings(12, 4, 2, 2) == (True, False, False) and walk_crossings(4, 2, 1, 1) == (False, True, False)
    v = valu_fwd_walk(64, 56, 56, 96)  # 28 8x16 tiles per image, halved twice: 256 walks x 3 channel blocks = 768 workgroups
    assert (v["ntile"], v["per"]) == (1792, 7) and valu_fwd_walk(1, 56, 56, 32)["per"] == 1
    assert valu_wgrad_walk(64, 56, 56, 96)["per"] == 7 and valu_wgrad_walk(2, 28, 28, 96)["per"] == 1
