"""The references of tests/input_pipeline_ref.py against what is already pinned to the reference implementation: oracle/aug_oracle.py,
oracle/mformer_oracle.py and the fixtures tests/golden/aug.npz / collate.npz.  Runs on the CPU.  The last part recomputes, from the
references alone, the figures the affine GPU tests assert (no tie in the exact transforms, at most 1 % of near-tie pixels and
more than 2 % of zero fill in the large ones)."""
import numpy as np
import pytest
import torch

from linnaeus_amd.aug import inverse_affine_matrix
from oracle import aug_oracle as A
from tests import input_pipeline_ref as R


def _z(golden_dir):
    return np.load(f"{golden_dir}/aug.npz", allow_pickle=False)


def _img(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 1.4 - 0.2  # values on both sides of [0, 1]


def _within(got, ref64, bound, what):
    assert bool(((got.double() - ref64).abs() <= bound).all()), what


def test_point_op_against_fixture_and_oracle(golden_dir):
    z = _z(golden_dir)
    img = torch.from_numpy(z["img"])
    args = {"Posterize": lambda m: (R.POSTERIZE, R.f32(2.0 ** m), 0.0), "PosterizeOriginal": lambda m: (R.POSTERIZE, R.f32(2.0 ** m), 0.0),
            "PosterizeIncreasing": lambda m: (R.POSTERIZE, R.f32(2.0 ** (8 - m)), 0.0), "Solarize": lambda m: (R.SOLARIZE, R.f32(m), 0.0),
            "SolarizeAdd": lambda m: (R.SOLARIZE_ADD, R.f32(m), 0.5), "Invert": lambda m: (R.INVERT, 0.0, 0.0)}
    for key in z["working_ops"]:
        name, m = str(key).split(":")
        op, p0, p1 = args[name](int(m) * 0.1)
        want, bound = R.point_op(img, op, p0, p1)
        assert bound is None and torch.equal(want, torch.from_numpy(z[f"op_{name}_{m}"])), key
    x = _img(1, 5, 3, 6, 6)
    for m in range(11):  # every magnitude of the three posterize operations
        for bits in (m * 0.1, 8 - m * 0.1):
            assert torch.equal(R.point_op(x, R.POSTERIZE, R.f32(2.0 ** bits))[0], A.posterize(x, bits)), bits
    assert torch.equal(R.point_op(x, R.CLAMP)[0], x.clamp(0, 1))
    assert torch.equal(R.point_op(x, R.BRIGHTNESS, 1.5)[0], A.brightness(x, 1.5))
    for f in (1.5, 0.5, 0.0):  # 1 - f exact, so the oracle's double 1 - f is the kernels' fp32 one
        want, bound = R.point_op(x, R.CONTRAST, f, 0.0, R.row_grey_mean(x.reshape(5, 3, 36))[0])
        _within(A.contrast(x, f), want, bound + abs(1 - f) * R.row_grey_mean(x.reshape(5, 3, 36))[1][:, None, None, None], f"contrast {f}")


def test_saturation_rowstat_rescale_against_oracle():
    x = _img(2, 4, 3, 9, 7)
    for f in (1.5, 0.5, 0.0, 1.0, -0.5):
        want, bound = R.saturation(x.reshape(4, 3, 63), f)
        _within(A.saturation(x, f).reshape(4, 3, 63), want, bound, f"saturation {f}")
    assert torch.equal(R.saturation(x.reshape(4, 3, 63), 1.0)[0].float(), x.reshape(4, 3, 63).clamp(0, 1))
    mean, bound = R.row_grey_mean(x.reshape(4, 3, 63))
    _within(A.grey(x).mean(dim=(1, 2, 3)), mean, bound, "mean grey level")
    rows = x.reshape(12, 63)
    assert torch.equal(R.row_minmax(rows), torch.stack([x.amin(dim=(2, 3)).reshape(12), x.amax(dim=(2, 3)).reshape(12)], 1))
    assert torch.equal(R.rescale(rows).reshape(x.shape), A.autocontrast(x))
    assert torch.equal(R.rescale(x.reshape(1, -1)).reshape(x.shape), A.equalize(x))
    assert torch.equal(R.rescale(torch.full((2, 5), 0.3)), torch.zeros(2, 5))


def test_stencil_against_oracle():
    import math

    x = _img(3, 2, 3, 19, 23)
    planes = x.reshape(6, 19, 23)
    sharp = torch.tensor([[1.0, 1.0, 1.0], [1.0, 5.0, 1.0], [1.0, 1.0, 1.0]]) / 13.0
    for ratio in (0.5, 0.0, 1.0, 1.5):
        want, bound = R.stencil(planes, sharp, 1, ratio)
        _within(A.sharpness(x, ratio).reshape(6, 19, 23), want, bound, f"sharpness {ratio}")
    for sigma, k in ((0.5, 3), (0.7, 5), (1.0, 7)):
        half = (k - 1) * 0.5
        g = torch.tensor([math.exp(-0.5 * ((i - half) / sigma) ** 2) for i in range(k)])
        g = g / g.sum()
        want, bound = R.stencil(planes, torch.outer(g, g), 0, 0.0)
        _within(A.gaussian_blur(x, sigma).reshape(6, 19, 23), want, bound, f"gaussian blur k = {k}")
    # the smallest image a 7 x 7 stencil takes: the reflection of every border reaches the far edge
    small = _img(4, 1, 1, 4, 4)
    g = torch.tensor([math.exp(-0.5 * (i - 3.0) ** 2) for i in range(7)])
    g = g / g.sum()
    want, bound = R.stencil(small.reshape(1, 4, 4), torch.outer(g, g), 0, 0.0)
    _within(A.gaussian_blur(small, 1.0).reshape(1, 4, 4), want, bound, "gaussian blur 4 x 4")


@pytest.mark.parametrize("mode", ["const", "rand"])
def test_erase_against_fixture(mode, golden_dir):
    """The rectangles of the reference's recorded draws, through erase(), give the reference's recorded output."""
    z = _z(golden_dir)
    img = torch.from_numpy(z["re_img"])
    B, C, H, W = img.shape
    for seed in (11, 12):
        out = img.clone()
        if float(z[f"re_{mode}_{seed}_gate"].reshape(-1)[0]) <= 0.9:
            for it in range(2):
                d = {k: torch.from_numpy(z[f"re_{mode}_{seed}_{it}_{k}"]) for k in ("areas", "aspects", "x", "y", "values")}
                h, w = torch.sqrt(d["areas"] * d["aspects"]).round().long(), torch.sqrt(d["areas"] / d["aspects"]).round().long()
                valid = (w < W) & (h < H)
                rects = torch.stack([torch.arange(B), d["y"].long(), d["x"].long(), torch.where(valid, h, 0), torch.where(valid, w, 0)], 1)
                out = R.erase(out, rects, d["values"].reshape(B, C))
        assert torch.equal(out.clamp(0, 1), torch.from_numpy(z[f"re_{mode}_{seed}_out"])), seed


def test_erase_clips_and_skips():
    x = torch.zeros(2, 1, 4, 5)
    rects = [[2, 0, 0, 2, 2], [-1, 0, 0, 2, 2], [0, 1, 1, 0, 3], [0, 1, 1, 3, -1], [0, -1, -2, 3, 4], [1, 3, 4, 9, 9], [1, 4, 0, 2, 2]]
    vals = torch.arange(1.0, 8.0).reshape(7, 1)
    want = torch.zeros(2, 1, 4, 5)
    want[0, 0, 0:2, 0:2] = 5.0
    want[1, 0, 3, 4] = 6.0
    assert torch.equal(R.erase(x, rects, vals), want)


def test_u8_to_f32_is_the_correctly_rounded_quotient():
    raw = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16, 1)
    want = (np.arange(256, dtype=np.float32) / np.float32(255.0)).reshape(1, 1, 16, 16)
    assert np.array_equal(R.u8_to_f32(raw).numpy(), want)


@pytest.mark.parametrize("name", ["mixup", "cutmix"])
def test_mix_meta_against_fixture(name, golden_dir):
    z = np.load(f"{golden_dir}/collate.npz")
    aux, masks = torch.from_numpy(z["aux"]), torch.from_numpy(z["masks"])
    oa, om = R.mix_meta(aux, masks, torch.from_numpy(z[f"{name}_perm"]), torch.from_numpy(z[f"{name}_pick"]), z["bounds"].tolist())
    assert torch.equal(oa, torch.from_numpy(z[f"{name}_aux"]))
    assert np.array_equal(om.numpy().astype(bool), z[f"{name}_masks"])


# --- affine: the figures the GPU tests assert, from the references alone ---------------------------------------------------------
def _affine_pair(H, W, kw, seed=5):
    x = torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.1  # no zero in the image: a zero is fill
    m6 = inverse_affine_matrix(kw.get("angle", 0.0), kw.get("translate", (0.0, 0.0)), kw.get("shear", (0.0, 0.0)))
    y, sx, sy = R.affine_gather(x.reshape(12, H, W), m6)
    return y.reshape(x.shape), A.affine(x, m6), R.near_tie(sx, sy)


@pytest.mark.parametrize("H,W", R.AFFINE_EXACT_SIZES)
def test_affine_exact_transforms_have_no_tie(H, W):
    for kw in R.affine_exact(W):
        y, want, tie = _affine_pair(H, W, kw)
        assert not bool(tie.any()) and torch.equal(y, want), kw
    y, _, _ = _affine_pair(H, W, dict(angle=180.0))
    x = torch.rand(4, 3, H, W, generator=torch.Generator().manual_seed(5)) * 0.9 + 0.1
    assert torch.equal(y, x.flip(2, 3))
    assert torch.equal(_affine_pair(H, W, dict(translate=(-float(W), 0.0)))[0], torch.zeros_like(x))


def test_affine_autoaug_range_has_no_tie():
    for kw in R.affine_autoaug(28):
        y, want, tie = _affine_pair(36, 28, kw)
        assert not bool(tie.any()) and torch.equal(y, want), kw


@pytest.mark.parametrize("H,W", R.AFFINE_LARGE_SIZES)
@pytest.mark.parametrize("kw", R.AFFINE_LARGE, ids=["rot-33", "shear25-10", "combined"])
def test_affine_large_transforms_cap(kw, H, W):
    y, want, tie = _affine_pair(H, W, kw)
    assert torch.equal(y[..., ~tie], want[..., ~tie])
    share, zero = float(tie.float().mean()), float((want == 0).float().mean())
    print(f"{kw} on {H} x {W}: {share:.4%} of pixels in the near-tie band, {zero:.2%} zero fill")
    assert share <= R.AFFINE_TIE_CAP and zero > R.AFFINE_ZERO_FLOOR
