"""Kernel-level tests of the input pipeline: the eight kernels of csrc/aug.hip behind GPUAutoAugmentBatch, GPURandomErasing and
u8hwc_to_f32chw, and mix_meta_kernel of csrc/collate.hip, against the plain torch references of tests/input_pipeline_ref.py.

Method (that of tests/test_gpu_data_movement.py): seeded inputs, every output inside a canary-guarded buffer, overwritten outputs
prefilled with NaN, the C entry points called directly so that odd shapes reach the kernels.  Tolerances: selections, copies and
single roundings are compared BIT FOR BIT; contrast, saturation, the mean grey level and the stencil use the derived bounds of
input_pipeline_ref (built from data_movement_ref's fma_bound, blend_bound, summation_bound) and nothing measured.  The only pixels
left out of any comparison are the near ties of the three large affine transforms, and their share is capped."""
import ctypes as C

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd.aug import inverse_affine_matrix
from oracle import aug_oracle as A
from tests import input_pipeline_ref as R
from tests.test_gpu_data_movement import CANARY, NAN, assert_bits, assert_within, cgen, flat

pytestmark = pytest.mark.gpu
GRID_CAP = 4096 * 256  # threads of the largest grid the aug kernels launch: more work items than this need a second pass


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def spread(gen, *shape):
    """Uniform in [-0.2, 1.2): both clamps are taken."""
    return torch.rand(*shape, generator=gen, device="cuda") * 1.4 - 0.2


def held(t):
    """t in a canary-guarded buffer (for the kernels that work in place)."""
    return flat(t.numel(), t.dtype, t.reshape(-1), tuple(t.shape))


def compare(got, want, bound, what):
    if bound is None:
        assert_bits(got, want, what)
    else:
        assert_within(got, want, bound, what)


class ByteGuard:
    """n bytes of 0x5A between two runs of 64 bytes of 0xA5."""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.big = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device="cuda")
        self.big[64:64 + n] = 0x5A
        self.win = self.big[64:64 + n].view(shape)

    def assert_canaries(self):
        assert bool((self.big[:64] == 0xA5).all()) and bool((self.big[-64:] == 0xA5).all()), "bytes outside the output window were written"


def test_operation_codes_are_the_library_s():
    assert (R.CLAMP, R.POSTERIZE, R.SOLARIZE, R.SOLARIZE_ADD, R.INVERT, R.BRIGHTNESS, R.CONTRAST) == (
        L.AUG_CLAMP, L.AUG_POSTERIZE, L.AUG_SOLARIZE, L.AUG_SOLARIZE_ADD, L.AUG_INVERT, L.AUG_BRIGHTNESS, L.AUG_CONTRAST)


# =====================================================================================================================================
# 1. lnx_aug_pointwise
# =====================================================================================================================================
def pointwise(x, op, p0=0.0, p1=0.0, per_image=0, per_img=None):
    L.check(L.lib().lnx_aug_pointwise(_p(x), C.c_int64(x.numel()), C.c_int64(per_image), op, C.c_float(p0), C.c_float(p1), _p(per_img), _stream()),
            "lnx_aug_pointwise")
    torch.cuda.synchronize()


# (name, op, p0, p1): the scalars are fp32 values, so c_float passes them on unchanged
POINT_OPS = [("clamp", R.CLAMP, 0.0, 0.0), ("posterize", R.POSTERIZE, R.f32(2.0 ** 0.8), 0.0), ("posterize_inc", R.POSTERIZE, R.f32(2.0 ** 7.4), 0.0),
             ("solarize", R.SOLARIZE, R.f32(0.6), 0.0), ("solarize_add", R.SOLARIZE_ADD, R.f32(0.3), 0.5), ("invert", R.INVERT, 0.0, 0.0),
             ("brightness", R.BRIGHTNESS, R.f32(1.6), 0.0), ("contrast", R.CONTRAST, R.f32(1.8), 0.0)]
POINT = pytest.mark.parametrize("name,op,p0,p1", POINT_OPS, ids=[o[0] for o in POINT_OPS])


@POINT
@pytest.mark.parametrize("n", [105, 3])
def test_pointwise_vectors_and_tail(n, name, op, p0, p1):
    """n = 105 (a 1 x 3 x 5 x 7 image): 26 vectors and a one-element tail; n = 3: the tail alone.  No per-image scalar can come with
    a tail (it needs per_image % 4 == 0), so contrast blends with s = 0 here.  The first and the last tail element lie outside
    [0, 1]: every operation ends in the clamp, so an element the kernel skipped cannot compare equal."""
    x0 = spread(cgen(n + op), n)
    x0[n & ~3], x0[n - 1] = (-0.15, 1.15) if (n & 3) > 1 else (1.15, 1.15)
    x = held(x0)
    pointwise(x.win, op, p0, p1)
    compare(x.win[None], *R.point_op(x0[None], op, p0, p1), name)  # [1, n]: one image
    x.assert_canaries()


@POINT
def test_pointwise_second_grid_stride_pass(name, op, p0, p1):
    """28 x 3 x 224 x 224 = 4 214 784 elements = 1 053 696 vectors > 4096 * 256: the first 5120 threads run a second pass.  Contrast
    takes 28 given per-image scalars (exact inputs: the bound is the blend's alone)."""
    B, per = 28, 3 * 224 * 224
    assert B * per // 4 > GRID_CAP
    gen = cgen(11 + op)
    x0 = spread(gen, B, per)
    s = torch.rand(B, generator=gen, device="cuda") if op == R.CONTRAST else None
    x = held(x0)
    pointwise(x.win, op, p0, p1, per, s)
    want, bound = R.point_op(x0, op, p0, p1, s)
    compare(x.win, want, bound, name)
    x.assert_canaries()


def grey_mean(x, rows, cols):
    out = flat(rows, torch.float32, NAN)
    L.check(L.lib().lnx_aug_rowstat(_p(x), rows, C.c_int64(cols), 1, _p(out.win), _stream()), "lnx_aug_rowstat")
    torch.cuda.synchronize()
    out.assert_canaries()
    return out.win


def test_contrast_image_boundaries_inside_a_wave():
    """B = 5 images of 3 x 6 x 6 = 27 vectors each: lanes 27, 54, ... of the first waves start a new image.  The mean grey levels are
    about 0.05, 0.95, 0.5 and exactly 0 and 1, so the scalar of a neighbouring image cannot pass.  As GPUAutoAugmentBatch._contrast
    runs it: lnx_aug_rowstat (kind 1), then the blend; the mean's own summation_bound enters times |1 - p0|."""
    B, hw = 5, 36
    gen = cgen(21)
    noise = (torch.rand(B, 3, hw, generator=gen, device="cuda") - 0.5) * 0.08
    level = torch.tensor([0.05, 0.95, 0.5, 0.0, 1.0], device="cuda")[:, None, None]
    x0 = level + noise * ((level > 0) & (level < 1))  # the last two images are constant 0 and constant 1
    for p0 in (R.f32(1.8), R.f32(0.1), 0.0):
        x = held(x0)
        mean = grey_mean(x.win, B, hw)
        mref, mbound = R.row_grey_mean(x0)
        assert_within(mean, mref, mbound, "mean grey level")
        assert float((mref - torch.tensor([0.05, 0.95, 0.5, 0.0, 1.0], device="cuda").double()).abs().max()) < 0.02
        pointwise(x.win, R.CONTRAST, p0, 0.0, 3 * hw, mean)
        want, bound = R.point_op(x0, R.CONTRAST, p0, 0.0, mref)
        assert_within(x.win, want, bound + abs(R.one_minus(p0)) * mbound[:, None, None], f"contrast {p0}")
        x.assert_canaries()


def test_solarize_at_the_threshold():
    """Values exactly at, one ulp below and one ulp above the threshold (x < t selects), for Solarize and SolarizeAdd."""
    for t in (0.5, R.f32(0.3), R.f32(0.7), 1.0):
        tt = torch.tensor(t, device="cuda")
        x0 = torch.stack([torch.nextafter(tt, tt - 1), tt, torch.nextafter(tt, tt + 1)]).repeat(7)  # 21 elements: vectors and a tail
        assert x0[0] < x0[1] < x0[2]
        for op, p0, p1 in ((R.SOLARIZE, t, 0.0), (R.SOLARIZE_ADD, R.f32(0.2), t)):
            x = held(x0)
            pointwise(x.win, op, p0, p1)
            want, _ = R.point_op(x0, op, p0, p1)
            assert_bits(x.win, want, f"op {op} at threshold {t}")
            if not (op == R.SOLARIZE_ADD and t == 1.0):  # (there both sides clamp to 1)
                assert not torch.equal(want[0:1], want[1:2])  # the threshold does separate the neighbours
            x.assert_canaries()


def test_posterize_every_magnitude_on_the_byte_levels():
    """Magnitudes 0..10 of Posterize, PosterizeOriginal (2^(0.1 m)) and PosterizeIncreasing (2^(8 - 0.1 m)) on the 256 levels k / 255
    and their ulp neighbours (where floor() flips), against aug_oracle.posterize on the CPU."""
    k = torch.arange(256, dtype=torch.float32) / torch.tensor(255.0)
    x0 = torch.cat([torch.nextafter(k, k - 1), k, torch.nextafter(k, k + 1)])
    for name, bits in [(n, m * 0.1) for n in ("Posterize", "PosterizeOriginal") for m in range(11)] + [("PosterizeIncreasing", 8 - m * 0.1) for m in range(11)]:
        x = held(x0.cuda())
        pointwise(x.win, R.POSTERIZE, 2.0 ** bits)
        assert_bits(x.win.cpu(), A.posterize(x0, bits), f"{name}, 2^{bits}")
        x.assert_canaries()


def test_pointwise_refusals():
    x0 = spread(cgen(31), 64)
    x = held(x0)
    s = torch.rand(4, device="cuda")
    lib = L.lib()

    def rc(xt, n, per, op, p0, sc):
        return lib.lnx_aug_pointwise(_p(xt), C.c_int64(n), C.c_int64(per), op, C.c_float(p0), C.c_float(0.0), _p(sc), _stream())

    with pytest.raises(L.LnxError, match="unknown operation"):
        L.check(rc(x.win, 64, 0, 7, 0.0, None), "lnx_aug_pointwise")
    with pytest.raises(L.LnxError, match="unknown operation"):
        L.check(rc(x.win, 64, 0, -1, 0.0, None), "lnx_aug_pointwise")
    with pytest.raises(L.LnxError, match="16-byte aligned"):
        L.check(rc(x.win[1:], 60, 0, R.INVERT, 0.0, None), "lnx_aug_pointwise")
    with pytest.raises(L.LnxError, match="multiple of 4"):
        L.check(rc(x.win, 60, 6, R.CONTRAST, 1.5, s), "lnx_aug_pointwise")
    for p0 in (0.0, -2.0):
        with pytest.raises(L.LnxError, match="posterize"):
            L.check(rc(x.win, 64, 0, R.POSTERIZE, p0, None), "lnx_aug_pointwise")
    torch.cuda.synchronize()
    assert_bits(x.win, x0, "a refused call wrote")
    x.assert_canaries()


# =====================================================================================================================================
# 2. lnx_aug_saturation
# =====================================================================================================================================
# hw = 1; 255 (one short of a workgroup); 50 177 = 224 * 224 + 1 (odd: no plane is 16-byte aligned); 21 * 50 177 > 4096 * 256
@pytest.mark.parametrize("f", [0.0, 1.0, R.f32(1.9), -0.5])
@pytest.mark.parametrize("B,hw", [(3, 1), (3, 255), (2, 50177), (21, 50177)])
def test_saturation(B, hw, f):
    assert (B, hw) != (21, 50177) or B * hw > GRID_CAP
    x0 = spread(cgen(B + hw), B, 3, hw)
    x = held(x0)
    L.check(L.lib().lnx_aug_saturation(_p(x.win), B, C.c_int64(hw), C.c_float(f), _stream()), "lnx_aug_saturation")
    torch.cuda.synchronize()
    assert_within(x.win, *R.saturation(x0, f), f"saturation {f}")
    if f == 1.0:  # 1 c + 0 grey: the clamped input itself
        assert_bits(x.win, x0.clamp(0, 1), "saturation 1")
    x.assert_canaries()


# =====================================================================================================================================
# 3. lnx_aug_rowstat
# =====================================================================================================================================
ROWSTAT = pytest.mark.parametrize("cols", [1, 63, 64, 255, 256, 257, 1000])
ROWS = pytest.mark.parametrize("rows", [1, 3, 770])


@ROWSTAT
@ROWS
def test_rowstat_min_max(rows, cols):
    """Exact.  Three launches, so that every row index sees every pattern: the minimum in the first and the maximum in the last
    element, the reverse, and a constant row."""
    lo, hi = -3.0, 5.0
    base = torch.rand(rows, cols, generator=cgen(rows + cols), device="cuda")
    for shift in range(3):
        x0 = base.clone()
        pat = (torch.arange(rows, device="cuda") + shift) % 3
        x0[pat == 0, 0], x0[pat == 0, -1] = lo, hi
        x0[pat == 1, 0], x0[pat == 1, -1] = hi, lo
        x0[pat == 2] = 0.25
        if cols == 1:
            x0[:, 0] = (pat.float() - 1) * 2.5  # one element: minimum = maximum
        out = flat(2 * rows, torch.float32, NAN, (rows, 2))
        L.check(L.lib().lnx_aug_rowstat(_p(x0), rows, C.c_int64(cols), 0, _p(out.win), _stream()), "lnx_aug_rowstat")
        torch.cuda.synchronize()
        assert_bits(out.win, R.row_minmax(x0), f"min / max, shift {shift}")
        out.assert_canaries()


@ROWSTAT
@ROWS
def test_rowstat_mean_grey_level(rows, cols):
    """Random images, then images of three constant planes with different values: permuted weights give another mean."""
    gen = cgen(3 * rows + cols)
    const = torch.tensor([0.2, 0.5, 0.9], device="cuda")[None, :, None].expand(rows, 3, cols).contiguous()
    for x0 in (spread(gen, rows, 3, cols), const):
        got = grey_mean(x0, rows, cols)
        assert_within(got, *R.row_grey_mean(x0), "mean grey level")
    w = R.grey_weights(const)
    others = [float((w[list(p)] * const[0, :, 0].double()).sum()) for p in ((0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))]
    ref, bound = R.row_grey_mean(const)
    assert min(abs(o - float(ref[0])) for o in others) > 100 * float(bound[0])  # the bound does tell the permutations apart


# =====================================================================================================================================
# 4. lnx_aug_rescale
# =====================================================================================================================================
# 9 rows of 7 (a row boundary every 7 lanes); 5 * 209 953 = 1 049 765 > 4096 * 256
@pytest.mark.parametrize("rows,cols", [(9, 7), (5, 209953)])
def test_rescale(rows, cols):
    """Exact.  Row r spans [10 r, 10 r + r + 1] (disjoint ranges: the minimum / maximum of another row clamps the whole row to 0 or
    1), row 2 is constant and must come out as zeros."""
    assert (rows, cols) == (9, 7) or rows * cols > GRID_CAP
    r = torch.arange(rows, device="cuda", dtype=torch.float32)[:, None]
    x0 = 10 * r + (r + 1) * torch.rand(rows, cols, generator=cgen(rows), device="cuda")
    x0[2] = 20.5
    mm = R.row_minmax(x0).contiguous()
    x = held(x0)
    L.check(L.lib().lnx_aug_rescale(_p(x.win), C.c_int64(rows), C.c_int64(cols), _p(mm), _stream()), "lnx_aug_rescale")
    torch.cuda.synchronize()
    want = R.rescale(x0)
    assert_bits(x.win, want, "rescale")
    assert float(want[2].abs().max()) == 0.0 and float(want[1].max()) > 0.9 and float(want[1].min()) < 0.1
    x.assert_canaries()


# =====================================================================================================================================
# 5. lnx_aug_stencil
# =====================================================================================================================================
def stencil(x, y, taps, k, mode, ratio):
    P, H, W = x.shape
    return L.lib().lnx_aug_stencil(_p(x), _p(y), P, H, W, _p(taps), k, mode, C.c_float(ratio), _stream())


@pytest.mark.parametrize("mode", [0, 1], ids=["reflect", "keep_border"])
@pytest.mark.parametrize("k", [1, 3, 5, 7, 9, 15])
def test_stencil(k, mode):
    """7 planes; (k//2 + 1)^2 is the smallest image the entry takes (mode 0: the reflection of every border reaches the far edge,
    mode 1: all border), (k//2 + 1) x (k + 6) has an interior in one direction only, 19 x 23 in both.  The taps are random, of both
    signs and without any symmetry: a transposed or flipped table gives other values."""
    r = k // 2
    gen = cgen(40 + k + mode)
    taps = (torch.randn(k, k, generator=gen, device="cuda") / k).contiguous()
    for H, W in ((r + 1, r + 1), (r + 1, k + 6), (19, 23)):
        x0 = spread(gen, 7, H, W)
        for ratio in (0.0, R.f32(0.7), 1.0):
            y = flat(x0.numel(), torch.float32, NAN, (7, H, W))
            L.check(stencil(x0, y.win, taps, k, mode, ratio), "lnx_aug_stencil")
            torch.cuda.synchronize()
            assert_within(y.win, *R.stencil(x0, taps, mode, ratio), f"stencil {H} x {W}, ratio {ratio}")
            y.assert_canaries()


def test_stencil_refusals():
    x = spread(cgen(49), 2, 8, 8)
    y = flat(x.numel(), torch.float32, NAN, (2, 8, 8))
    taps = torch.ones(17 * 17, device="cuda")
    for k, xs, ys in ((4, x, y.win), (17, x, y.win), (7, x[:, :3].contiguous(), y.win), (7, x[:, :, :3].contiguous(), y.win), (3, x, x)):
        with pytest.raises(L.LnxError, match="lnx_aug_stencil"):
            L.check(stencil(xs, ys, taps, k, 0, 0.5), "lnx_aug_stencil")
    with pytest.raises(L.LnxError, match="mode"):
        L.check(stencil(x, y.win, taps, 3, 2, 0.5), "lnx_aug_stencil")
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.win).all())
    y.assert_canaries()


# =====================================================================================================================================
# 6. lnx_aug_affine
# =====================================================================================================================================
def m6_of(kw):
    return inverse_affine_matrix(kw.get("angle", 0.0), kw.get("translate", (0.0, 0.0)), kw.get("shear", (0.0, 0.0)))


def affine(x0, m6):
    """x0 [planes, H, W] -> the guarded output of lnx_aug_affine."""
    P, H, W = x0.shape
    y = flat(x0.numel(), torch.float32, NAN, (P, H, W))
    L.check(L.lib().lnx_aug_affine(_p(x0), _p(y.win), P, H, W, (C.c_float * 6)(*m6), _stream()), "lnx_aug_affine")
    torch.cuda.synchronize()
    y.assert_canaries()
    return y.win


def image(seed, P, H, W):
    """(0.1, 1]: no zero in the image, so a zero in the output is fill."""
    return torch.rand(P, H, W, generator=cgen(seed), device="cuda") * 0.9 + 0.1


@pytest.mark.parametrize("H,W", R.AFFINE_EXACT_SIZES)
def test_affine_exact_transforms(H, W):
    """The identity, integer translations and quarter turns have no source coordinate near a tie (tests/test_input_pipeline_ref.py):
    equal to the direct gather bit for bit, everywhere."""
    x0 = image(H, 5, H, W)
    for kw in R.affine_exact(W):
        want, sx, sy = R.affine_gather(x0, m6_of(kw))
        assert not bool(R.near_tie(sx, sy).any())
        assert_bits(affine(x0, m6_of(kw)), want, f"{kw}")
    assert_bits(affine(x0, m6_of(dict())), x0, "identity")
    assert_bits(affine(x0, m6_of(dict(angle=180.0))), x0.flip(1, 2), "half turn")
    assert_bits(affine(x0, m6_of(dict(translate=(-float(W), 0.0)))), torch.zeros_like(x0), "translated out of the image")
    shifted = torch.zeros_like(x0)
    shifted[:, :H - 2, 3:] = x0[:, 2:, :W - 3]  # translate = (3, -2): 3 right, 2 up
    assert_bits(affine(x0, m6_of(dict(translate=(3.0, -2.0)))), shifted, "translation by (3, -2)")


def test_affine_autoaug_range_equals_the_oracle():
    """The largest transforms AutoAugment reaches: equal to aug_oracle.affine and to the direct gather everywhere (no tie exists)."""
    x0 = image(61, 12, 36, 28)
    for kw in R.affine_autoaug(28):
        got = affine(x0, m6_of(kw))
        assert_bits(got, R.affine_gather(x0, m6_of(kw))[0], f"{kw} against the gather")
        assert_bits(got.cpu(), A.affine(x0.cpu().reshape(4, 3, 36, 28), m6_of(kw)).reshape(12, 36, 28), f"{kw} against the oracle")


# The half-pixel translation (magnitude 5 of TranslateX / TranslateY) is not a case: every pixel is an exact tie there and the
# parity of the result is undefined.
@pytest.mark.parametrize("H,W", R.AFFINE_LARGE_SIZES)
@pytest.mark.parametrize("kw", R.AFFINE_LARGE, ids=["rot-33", "shear25-10", "combined"])
def test_affine_large_transforms(kw, H, W):
    """Equal to aug_oracle.affine (and to the direct gather) on every pixel whose float64 source coordinate is more than 1e-3 away
    from k + 0.5 in x and y; at most 1 % of the pixels are that close, more than 2 % are zero fill."""
    x0 = image(H + W, 12, H, W)
    m6 = m6_of(kw)
    got = affine(x0, m6)
    gather, sx, sy = R.affine_gather(x0, m6)
    tie = R.near_tie(sx, sy)
    oracle = A.affine(x0.cpu().reshape(4, 3, H, W), m6).reshape(12, H, W).cuda()
    share, zero = float(tie.float().mean()), float((oracle == 0).float().mean())
    print(f"{kw} on {H} x {W}: {share:.4%} near ties, {zero:.2%} zero fill, {int((got != oracle).sum())} pixels differ from the oracle")
    assert share <= R.AFFINE_TIE_CAP and zero > R.AFFINE_ZERO_FLOOR
    assert_bits(got[:, ~tie], oracle[:, ~tie], "against the oracle")
    assert_bits(got[:, ~tie], gather[:, ~tie], "against the gather")


def test_affine_second_grid_stride_pass():
    """5 x 459 x 459 = 1 053 405 > 4096 * 256 pixels; a quarter turn, which is exact."""
    P, H = 5, 459
    assert P * H * H > GRID_CAP
    x0 = image(71, P, H, H)
    m6 = m6_of(dict(angle=90.0))
    want, sx, sy = R.affine_gather(x0, m6)
    assert not bool(R.near_tie(sx, sy).any())
    assert_bits(affine(x0, m6), want, "quarter turn")


# =====================================================================================================================================
# 7. lnx_erase_rects
# =====================================================================================================================================
def erase_rects(x, rects, vals, n=None):
    B, Cn, H, W = x.shape
    return L.lib().lnx_erase_rects(_p(x), B, Cn, H, W, _p(rects), _p(vals), rects.shape[0] if n is None else n, _stream())


def guarded_batch(seed, B, Cn, H, W):
    """(buffer of B + 2 images, the batch = images 1..B of it): a canary image on either side."""
    buf = torch.full((B + 2, Cn, H, W), CANARY, device="cuda")
    buf[1:B + 1] = torch.rand(B, Cn, H, W, generator=cgen(seed), device="cuda")
    return buf, buf[1:B + 1]


def assert_guard_images(buf):
    assert bool((buf[0] == CANARY).all()) and bool((buf[-1] == CANARY).all()), "an image outside the batch was written"


def clipped(rect, H, W):
    _, y0, x0, h, w = rect
    return max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)


def test_erase_every_position_and_size():
    """Every rectangle with y0 in -2..6, x0 in -2..8 and (h, w) in {(1,1), (2,3), (6,8), (9,11)} on 2 x 3 x 6 x 8 images, each with
    values of its own.  Rectangles that overlap in one launch would race, so the 792 are packed greedily into launches of pairwise
    disjoint ones (empty after clipping = disjoint from everything); every launch is one bit-for-bit comparison."""
    B, Cn, H, W = 2, 3, 6, 8
    todo = [(b, y0, x0, h, w) for (h, w) in ((1, 1), (2, 3), (6, 8), (9, 11)) for y0 in range(-2, 7) for x0 in range(-2, 9) for b in range(B)]
    launches = []  # [rects, occupancy [B, H, W]]
    for rect in todo:
        ya, yb, xa, xb = clipped(rect, H, W)
        for rects, occ in launches:
            if ya >= yb or xa >= xb or not bool(occ[rect[0], ya:yb, xa:xb].any()):
                break
        else:
            rects, occ = [], torch.zeros(B, H, W, dtype=torch.bool)
            launches.append((rects, occ))
        rects.append(rect)
        if ya < yb and xa < xb:
            occ[rect[0], ya:yb, xa:xb] = True
    assert sum(len(r) for r, _ in launches) == 792 and max(len(r) for r, _ in launches) > 50
    gen = cgen(81)
    for i, (rects, _) in enumerate(launches):
        buf, x = guarded_batch(82, B, Cn, H, W)
        x0 = x.clone()
        rd = torch.tensor(rects, dtype=torch.int32, device="cuda")
        vals = 2.0 + torch.rand(len(rects), Cn, generator=gen, device="cuda")  # outside [0, 1): no value is an image's
        L.check(erase_rects(x, rd, vals), "lnx_erase_rects")
        torch.cuda.synchronize()
        assert_bits(x, R.erase(x0, rd.cpu(), vals), f"launch {i} of {len(rects)} rectangles")
        assert_guard_images(buf)


def test_erase_overlap_empty_list_and_list_length():
    B, Cn, H, W = 2, 3, 6, 8
    buf, x = guarded_batch(83, B, Cn, H, W)
    x0 = x.clone()
    # overlapping rectangles of one value: any write order gives the same image
    rd = torch.tensor([[0, 1, 1, 3, 4], [0, 2, 3, 3, 4], [1, -1, 5, 4, 9], [1, 0, 6, 6, 1]], dtype=torch.int32, device="cuda")
    vals = torch.tensor([[2.0, 3.0, 4.0]], device="cuda").repeat(4, 1)
    L.check(erase_rects(x, rd, vals), "lnx_erase_rects")
    torch.cuda.synchronize()
    want = R.erase(x0, rd.cpu(), vals)
    assert_bits(x, want, "overlapping rectangles")
    # n_rects = 0: nothing happens (and the lists are not looked at)
    L.check(erase_rects(x, rd, vals, 0), "lnx_erase_rects")
    L.check(L.lib().lnx_erase_rects(_p(x), B, Cn, H, W, None, None, 0, _stream()), "lnx_erase_rects")
    torch.cuda.synchronize()
    assert_bits(x, want, "n_rects = 0")
    # 65 535 rectangles (the y extent of a grid) are taken: all but three are skipped ones, the three sit at the ends and the middle
    n = 65535
    big = torch.tensor([[-1, 0, 0, 2, 2], [B, 0, 0, 2, 2], [0, 0, 0, 0, 2]], dtype=torch.int32, device="cuda").repeat(n // 3, 1)
    big[0], big[n // 2], big[n - 1] = torch.tensor([[0, 0, 0, 1, 1], [1, 5, 0, 1, 2], [0, 5, 7, 1, 1]], dtype=torch.int32, device="cuda")
    bvals = 2.0 + torch.rand(n, Cn, generator=cgen(84), device="cuda")
    L.check(erase_rects(x, big, bvals), "lnx_erase_rects")
    torch.cuda.synchronize()
    want = R.erase(want, big.cpu(), bvals)
    assert_bits(x, want, "65 535 rectangles")
    assert int((want != x0).sum()) > 3 * Cn
    with pytest.raises(L.LnxError, match="bad rectangle list"):
        L.check(erase_rects(x, big, bvals, 65536), "lnx_erase_rects")
    with pytest.raises(L.LnxError, match="bad rectangle list"):
        L.check(erase_rects(x, big, bvals, -1), "lnx_erase_rects")
    torch.cuda.synchronize()
    assert_bits(x, want, "a refused call wrote")
    assert_guard_images(buf)


def test_erase_rectangle_larger_than_one_pass():
    """3 x 38 x 39 = 4446 > 16 * 256 elements of one rectangle: its 16 workgroups loop."""
    buf, x = guarded_batch(85, 2, 3, 40, 41)
    x0 = x.clone()
    rd = torch.tensor([[1, 1, 1, 38, 39], [0, 35, -3, 9, 50]], dtype=torch.int32, device="cuda")
    vals = 2.0 + torch.rand(2, 3, generator=cgen(86), device="cuda")
    L.check(erase_rects(x, rd, vals), "lnx_erase_rects")
    torch.cuda.synchronize()
    assert_bits(x, R.erase(x0, rd.cpu(), vals), "large rectangle")
    assert_guard_images(buf)


# =====================================================================================================================================
# 8. lnx_u8hwc_to_f32chw
# =====================================================================================================================================
def u8_to_f32(raw):
    B, H, W, Cn = raw.shape
    out = flat(raw.numel(), torch.float32, NAN, (B, Cn, H, W))
    L.check(L.lib().lnx_u8hwc_to_f32chw(_p(raw), _p(out.win), B, H, W, Cn, _stream()), "lnx_u8hwc_to_f32chw")
    torch.cuda.synchronize()
    out.assert_canaries()
    return out.win


@pytest.mark.parametrize("Cn", [1, 3, 4])
def test_u8_to_f32_every_byte_in_every_channel(Cn):
    """2 x 8 x 16 = 256 pixels: every channel holds each byte value once (shifted by 37 per channel, so channels differ)."""
    B, H, W = 2, 8, 16
    raw = ((torch.arange(256)[:, None] + 37 * torch.arange(Cn)[None, :]) % 256).to(torch.uint8).reshape(B, H, W, Cn).cuda()
    for c in range(Cn):
        assert torch.equal(torch.sort(raw[..., c].reshape(-1).int()).values.cpu(), torch.arange(256, dtype=torch.int32))
    want = R.u8_to_f32(raw)
    assert_bits(u8_to_f32(raw), want, f"C = {Cn}")
    assert_bits(want.cpu(), raw.cpu().permute(0, 3, 1, 2).float() / 255, "the reference against the CPU's quotient")


def test_u8_to_f32_second_grid_stride_pass():
    B, H, W, Cn = 6, 250, 234, 3
    assert B * H * W * Cn > GRID_CAP
    raw = torch.randint(0, 256, (B, H, W, Cn), generator=cgen(91), device="cuda", dtype=torch.uint8)
    assert_bits(u8_to_f32(raw), R.u8_to_f32(raw), "u8 -> f32")


# =====================================================================================================================================
# 9. lnx_mix_meta
# =====================================================================================================================================
BELOW_HALF = float(torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)))  # the largest fp32 below 0.5
PICKS = [0.0, BELOW_HALF, 0.5, R.f32(0.99)]


def meta_batch(seed, B, D, bounds, shift):
    """aux without zeros except where a chunk is made absent by ONE zero (first, middle or last position of the chunk, as +0 or -0);
    presence is drawn per (sample, chunk); mask bytes are random everywhere (zeros inside present chunks included); the permutation
    is a cyclic shift (a derangement); the picks cycle through PICKS."""
    gen = torch.Generator().manual_seed(seed)
    aux = torch.randn(B, D, generator=gen)
    aux = torch.where(aux.abs() < 0.1, torch.ones(()), aux)
    present = torch.rand(B, len(bounds), generator=gen) < 0.5
    for b in range(B):
        for c, (s, e) in enumerate(bounds):
            if not present[b, c]:
                aux[b, (s, (s + e - 1) // 2, e - 1)[(b + c) % 3]] = -0.0 if (b // 3 + c) % 2 else 0.0
    masks = torch.rand(B, D, generator=gen) < 0.7
    perm = (torch.arange(B) + shift) % B
    pick = torch.tensor(PICKS)[torch.arange(B) % 4]
    assert not bool((perm == torch.arange(B)).any())
    return aux, masks, perm, pick, present


def run_mix_meta(aux, masks, perm, pick, bounds):
    B, D = aux.shape
    bd = torch.tensor([v for se in bounds for v in se], dtype=torch.int32, device="cuda")
    oa = flat(B * D, torch.float32, NAN, (B, D))
    om = ByteGuard((B, D))
    L.check(L.lib().lnx_mix_meta(_p(aux), _p(masks.view(torch.uint8)), _p(perm), _p(pick), _p(bd), len(bounds), B, D, _p(oa.win), _p(om.win), _stream()), "lnx_mix_meta")
    torch.cuda.synchronize()
    oa.assert_canaries()
    om.assert_canaries()
    return oa.win, om.win


def test_mix_meta_truth_table():
    """B = 100, chunks (0,2), (2,5), (5,15) of D = 15: 300 (sample, chunk) pairs, a second workgroup.  Every chunk sees own present /
    absent x partner present / absent under each of the four picks (0, the largest fp32 below 0.5, 0.5, 0.99).  Bit for bit
    against the oracle: an absent / absent chunk gives +0.0 and mask 0, every other the source row's values and mask bytes."""
    B, D, bounds = 100, 15, [(0, 2), (2, 5), (5, 15)]
    assert B * len(bounds) > 256
    aux, masks, perm, pick, present = meta_batch(95, B, D, bounds, 37)
    aux, masks, perm, pick = aux.cuda(), masks.cuda(), perm.cuda(), pick.cuda()
    for c in range(len(bounds)):
        seen = {(bool(present[b, c]), bool(present[int(perm[b]), c]), b % 4) for b in range(B)}
        assert len(seen) == 16, f"chunk {c}: only {len(seen)} of the 16 cases occur"
    assert int((torch.signbit(aux) & (aux == 0)).sum()) > 10 and int((~torch.signbit(aux) & (aux == 0)).sum()) > 10
    aux0, masks0 = aux.clone(), masks.clone()
    oa, om = run_mix_meta(aux, masks, perm, pick, bounds)
    wa, wm = R.mix_meta(aux, masks, perm, pick, bounds)
    assert_bits(oa, wa, "out_aux")
    assert torch.equal(om, wm.view(torch.uint8)), "out_mask"
    assert_bits(aux, aux0, "the input aux")
    assert torch.equal(masks, masks0), "the input mask"
    # the oracle's rows are what the truth table says (spot check of one sample per case of the last chunk)
    s, e = bounds[2]
    for b in range(16):
        own, other, p = bool(present[b, 2]), bool(present[int(perm[b]), 2]), float(pick[b])
        src = (b if p < 0.5 else int(perm[b])) if own and other else b if own else int(perm[b]) if other else None
        if src is None:
            assert int(R.bits(oa[b, s:e]).abs().sum()) == 0 and int(om[b, s:e].sum()) == 0
        else:
            assert torch.equal(oa[b, s:e], aux[src, s:e]) and torch.equal(om[b, s:e], masks[src, s:e].view(torch.uint8))


@pytest.mark.parametrize("D,bounds", [(1, [(0, 1)]), (15, [(0, 1), (1, 15)]), (6, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6)])])
def test_mix_meta_length_one_chunks(D, bounds):
    B = 40
    aux, masks, perm, pick = (t.cuda() for t in meta_batch(96 + D, B, D, bounds, 7)[:4])
    oa, om = run_mix_meta(aux, masks, perm, pick, bounds)
    wa, wm = R.mix_meta(aux, masks, perm, pick, bounds)
    assert_bits(oa, wa, "out_aux")
    assert torch.equal(om, wm.view(torch.uint8)), "out_mask"


def test_mix_meta_wrapper_keeps_uncovered_columns():
    """_SelectiveMixBase._mix_meta with bounds that leave columns 0, 3..5 and 9..11 uncovered: those keep the sample's own values and
    mask, the covered ones are the oracle's; the caller's tensors are unchanged."""
    from linnaeus_amd.collate import GPUSelectiveMixup

    B, D, bounds = 24, 12, [(1, 3), (6, 9)]
    aux, masks, perm, pick = (t.cuda() for t in meta_batch(99, B, D, bounds, 5)[:4])
    aux0, masks0 = aux.clone(), masks.clone()
    mix = GPUSelectiveMixup({"PROB": 1.0, "ALPHA": 0.4, "meta_chunk_bounds_list": [list(b) for b in bounds]})
    oa, om = mix._mix_meta(aux, masks, perm, pick)
    torch.cuda.synchronize()
    wa, wm = R.mix_meta(aux, masks, perm, pick, bounds)
    covered = torch.zeros(D, dtype=torch.bool, device="cuda")
    for s, e in bounds:
        covered[s:e] = True
    assert oa.dtype == aux.dtype and om.dtype == masks.dtype
    assert_bits(oa, torch.where(covered, wa, aux0), "mixed aux")
    assert torch.equal(om, torch.where(covered, wm, masks0)), "mixed mask"
    assert_bits(aux, aux0, "the caller's aux")
    assert torch.equal(masks, masks0), "the caller's mask"


# =====================================================================================================================================
# 10. the wrappers, exact values
# =====================================================================================================================================
@pytest.mark.parametrize("mode", ["const", "rand", "pixel"])
def test_random_erasing_batch_against_the_oracle(mode):
    """GPURandomErasing on B = 32 with injected draws against aug_oracle.random_erasing (which loops over the samples).  const and
    rand: exact, two rounds of rectangles.  pixel: the value is noise std + mean of the sample's channel, compared with the float64
    value within input_pipeline_ref.pixel_values' bound (one round: the statistics of a second would start from rounded pixels)."""
    from linnaeus_amd.aug import GPURandomErasing

    B, Cn, H, W = 32, 3, 48, 40
    cfg = {"PROB": 0.9, "AREA_RANGE": [0.02, 0.6], "ASPECT_RATIO": [0.3, 3.3], "COUNT": 1 if mode == "pixel" else 2, "MODE": mode}
    gen = torch.Generator().manual_seed(7)
    x0 = torch.rand(B, Cn, H, W, generator=gen)
    draws = []
    for it in range(cfg["COUNT"]):
        areas = torch.empty(B).uniform_(0.02 * H * W, 0.6 * H * W, generator=gen)
        aspects = torch.empty(B).uniform_(0.3, 3.3, generator=gen)
        h, w = torch.sqrt(areas * aspects).round().long(), torch.sqrt(areas / aspects).round().long()
        d = {"areas": areas, "aspects": aspects, "x": (torch.rand(B, generator=gen) * (W - w).clamp(min=1)).long(),
             "y": (torch.rand(B, generator=gen) * (H - h).clamp(min=1)).long(),
             "values": torch.randn(B, Cn, generator=gen) if mode == "pixel" else torch.rand(B, Cn, generator=gen)}
        assert 0 < int(((w >= W) | (h >= H)).sum()) < B // 2  # some samples draw a rectangle that does not fit and stay as they are
        draws.append(d)
    draws[0]["gate"] = torch.tensor([0.3])
    re = GPURandomErasing(cfg)
    re._draws = draws
    got = re(x0.cuda().clone()).cpu()
    if mode != "pixel":
        want = A.random_erasing(x0, draws, cfg)
        assert_bits(got, want, mode)
        assert int((want != x0).any(1).any(1).any(1).sum()) > B // 2
    else:
        want = A.random_erasing(x0.double(), draws, cfg)
        erased = want != x0.double()
        vals, bound = R.pixel_values(x0, draws[0]["values"])
        assert int(erased.any(3).any(2).all(1).sum()) > B // 2
        # two float64 evaluations of the same value: 2^-40 is far above their rounding and 2^-16 of fp32's unit roundoff
        assert_within(want, torch.where(erased, vals.clamp(0, 1)[:, :, None, None], x0.double()), torch.full((), 2.0 ** -40), "the oracle's values are pixel_values'")
        assert_within(got, want, torch.where(erased, bound[:, :, None, None], torch.zeros((), dtype=torch.float64)), mode)


def test_pipeline_rescales_0_255_input_exactly():
    """GPUAugmentationPipeline on a 0..255 batch gives, bit for bit, what it gives on the same batch divided by 255 beforehand."""
    from types import SimpleNamespace as NS

    from linnaeus_amd.aug import GPUAugmentationPipeline

    cfg = NS(AUG=NS(AUTOAUG=NS(POLICY="hybrid_v0", COLOR_JITTER=0.4),
                    RANDOM_ERASE={"PROB": 1.0, "AREA_RANGE": [0.02, 0.3], "ASPECT_RATIO": [0.3, 3.3], "COUNT": 2, "MODE": "pixel"}))
    pipe = GPUAugmentationPipeline(cfg)
    raw = torch.randint(0, 256, (8, 3, 32, 32), generator=cgen(97), device="cuda").float()
    outs = []
    for x in (raw, raw / 255.0):
        torch.manual_seed(13)
        outs.append(pipe((x, None, None))[0])
    assert_bits(outs[0], outs[1], "0..255 input against the input / 255")
    assert 0.0 <= float(outs[0].min()) and float(outs[0].max()) <= 1.0 and not torch.equal(outs[0], raw / 255.0)
