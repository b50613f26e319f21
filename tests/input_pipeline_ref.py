"""Plain torch restatement of the input-pipeline kernels (linnaeus_amd/csrc/aug.hip, mix_meta_kernel of csrc/collate.hip), for
tests/test_gpu_input_pipeline.py and tests/test_input_pipeline_ref.py.  Everything runs on whatever device its inputs live on.

Selections, copies and single roundings (clamp, posterize, solarize, solarize-add, invert, brightness, rescale, affine, erase,
u8 -> f32, mix_meta, row min / max) are stated as the same fp32 expression and compared bit for bit; where oracle/aug_oracle.py or
oracle/mformer_oracle.py already states the operation it is called, not restated.  The arithmetic ones (contrast, saturation, mean
grey level, stencil) return (float64 value, bound): the float64 value of the expression with the fp32 constants the kernels hold
(the grey weights, fp32(1 - factor)), and a bound built from tests/data_movement_ref.py (fma_bound, blend_bound, summation_bound).
A clamp to [0, 1] follows every operation; it never widens an error, so the bounds pass through it.

A division by a Python number is never used on a tensor here: torch may evaluate `t / 255` on a device as t * (1 / 255), which is
one rounding off the correctly rounded quotient the kernels (and the CPU) compute.  Divisors are 0-dim tensors on t's device."""
import torch

from oracle import aug_oracle as A
from oracle.mformer_oracle import _mix_meta_chunks
from tests.data_movement_ref import U, bits, blend_bound, fma_bound, summation_bound  # noqa: F401 (bits: for the tests)

# lnx_aug_pointwise operations (include/lnx.h)
CLAMP, POSTERIZE, SOLARIZE, SOLARIZE_ADD, INVERT, BRIGHTNESS, CONTRAST = range(7)
GREY = (0.2989, 0.587, 0.114)
BAND = 1e-3  # affine: a source coordinate this close to k + 0.5 is a near tie (see near_tie)

# affine cases, as keyword arguments of linnaeus_amd.aug.inverse_affine_matrix.  The half-pixel translation (magnitude 5 of
# TranslateX / TranslateY) is left out on purpose: every pixel is an exact tie there and the parity of the result is undefined.
AFFINE_EXACT_SIZES = [(17, 17), (8, 8)]


def affine_exact(W):
    """No source coordinate of these is anywhere near a tie: the results are defined everywhere."""
    return [dict(), dict(translate=(3.0, -2.0)), dict(translate=(-float(W), 0.0)), dict(angle=90.0), dict(angle=180.0), dict(angle=270.0)]


def affine_autoaug(W):
    """The largest transforms AutoAugment's magnitudes reach (ShearX 0.9, ShearY 0.4, TranslateX / Y 1.0, TranslateYRel 0.9,
    Rotate 0.9), on the 36 x 28 image of tests/test_aug.py."""
    return [dict(shear=(0.9, 0.0)), dict(shear=(0.0, 0.4)), dict(translate=(1.0, 0.0)), dict(translate=(0.0, 1.0)), dict(translate=(0.0, 0.9 * W)),
            dict(angle=-0.9)]


AFFINE_LARGE = [dict(angle=-33.0), dict(shear=(25.0, -10.0)), dict(angle=10.0, translate=(5.3, -7.1), shear=(8.0, 3.0))]
AFFINE_LARGE_SIZES = [(36, 28), (17, 23), (33, 33)]
AFFINE_TIE_CAP, AFFINE_ZERO_FLOOR = 0.01, 0.02  # at most 1 % of pixels in the band, more than 2 % zero fill


def f32(v):
    """The fp32 value nearest to the Python float v, as a Python float (what ctypes.c_float hands to a kernel)."""
    return float(torch.tensor(v, dtype=torch.float32))


def one_minus(f):
    """fp32(1 - fp32(f)) as a Python float: the second blend weight as the kernels compute it."""
    return float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(f, dtype=torch.float32))


def _s(v, like):
    return torch.tensor(v, dtype=like.dtype, device=like.device)


def grey_weights(like):
    """The three fp32 grey weights as float64, on like's device."""
    return torch.tensor(GREY, dtype=torch.float32, device=like.device).double()


# --- lnx_aug_pointwise --------------------------------------------------------------------------------------------------------------
def point_op(x, op, p0=0.0, p1=0.0, per_img=None):
    """(want, bound) of clamp(op(x)).  x fp32, any shape ([B, ...] with per_img [B]); p0 / p1 Python floats that are fp32 values.
    Every operation but CONTRAST: want is fp32 and bound is None (compare bit for bit).  CONTRAST, p0 x + fp32(1 - p0) s[image]:
    want is float64 and bound the blend_bound of the two terms; per_img is taken as exact (an error of it is the caller's to add,
    times |1 - p0|)."""
    if op == CLAMP:
        return A.clamp01(x), None
    if op == POSTERIZE:  # aug_oracle.posterize takes the bits, the kernel 2^bits: floor(x 255 / p0) p0 / 255, left to right
        q, c = _s(p0, x), _s(255.0, x)
        return A.clamp01(torch.floor(x * c / q) * q / c), None
    if op == SOLARIZE:
        return A.solarize(x, p0), None
    if op == SOLARIZE_ADD:
        return A.solarize_add(x, p0, p1), None
    if op == INVERT:
        return A.invert(x), None
    if op == BRIGHTNESS:
        return A.brightness(x, p0), None
    if op == CONTRAST:
        s = torch.zeros(x.shape[0], dtype=torch.float64, device=x.device) if per_img is None else per_img.double()
        a = x.double() * p0
        b = (one_minus(p0) * s).reshape(-1, *([1] * (x.dim() - 1))).expand_as(a)
        return A.clamp01(a + b), blend_bound(a, b)
    raise ValueError(f"unknown operation {op}")


# --- lnx_aug_saturation -------------------------------------------------------------------------------------------------------------
def saturation(x, f):
    """x [B, 3, hw] -> (float64 clamp(f c + fp32(1 - f) grey), bound).  The terms are f c and the three products that make up
    fp32(1 - f) grey; blend_bound of the four is 4 u of their magnitudes."""
    m = one_minus(f)
    x64, w = x.double(), grey_weights(x)
    a = x64 * f
    g = [(m * w[c] * x64[:, c:c + 1]).expand_as(a) for c in range(3)]
    return A.clamp01(a + g[0] + g[1] + g[2]), blend_bound(a, *g)


# --- lnx_aug_rowstat ----------------------------------------------------------------------------------------------------------------
def row_minmax(x):
    """x [rows, cols] -> fp32 [rows, 2] (min, max): selections, exact."""
    return torch.stack([x.amin(1), x.amax(1)], 1)


def row_grey_mean(x):
    """x [rows, 3, cols] -> (float64 mean grey level [rows], bound): a sum of 3 cols products, divided by cols."""
    cols = x.shape[2]
    terms = grey_weights(x)[None, :, None] * x.double()
    return terms.sum((1, 2)) / cols, summation_bound(3 * cols, terms.abs().sum((1, 2))) / cols


# --- lnx_aug_rescale ----------------------------------------------------------------------------------------------------------------
def rescale(x):
    """x [rows, cols] -> fp32 clamp((x - min_row) / (max_row - min_row + 1e-6)): aug_oracle.autocontrast with one row per (image,
    channel).  A subtraction, a sum and a correctly rounded quotient, none of which can be contracted: exact."""
    return A.autocontrast(x[None, :, None, :])[0, :, 0, :]


# --- lnx_aug_stencil ----------------------------------------------------------------------------------------------------------------
def _reflect(n, r, device):
    i = torch.arange(-r, n + r, device=device).abs()
    return torch.where(i > n - 1, 2 * (n - 1) - i, i)


def stencil(x, taps, mode, ratio):
    """x [planes, H, W], taps [k, k] (k odd) -> (float64 clamp(ratio x + fp32(1 - ratio) acc), bound).  Mode 0: acc = the
    correlation of the reflection-padded image with the taps.  Mode 1: the same where the whole window lies inside the image, and
    acc = x in the border of width k // 2.  Bound: |1 - ratio| times the summation_bound of the k k products, plus the blend_bound of
    the final mix."""
    k = taps.shape[0]
    r = k // 2
    P, H, W = x.shape
    x64, t64 = x.double(), taps.double()
    if mode == 0:
        src = x64[:, _reflect(H, r, x.device)][:, :, _reflect(W, r, x.device)]  # [P, H + 2r, W + 2r]
        oh, ow = H, W
    else:
        src = x64
        oh, ow = max(H - 2 * r, 0), max(W - 2 * r, 0)
    acc = torch.zeros(P, oh, ow, dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(acc)
    if oh > 0 and ow > 0:
        for i in range(k):
            for j in range(k):
                term = t64[i, j] * src[:, i:i + oh, j:j + ow]
                acc += term
                mag += term.abs()
    if mode == 1:
        full, fmag = x64.clone(), torch.zeros_like(x64)
        if oh > 0 and ow > 0:
            full[:, r:H - r, r:W - r], fmag[:, r:H - r, r:W - r] = acc, mag
        acc, mag = full, fmag
    m = one_minus(ratio)
    a, b = x64 * ratio, acc * m
    return A.clamp01(a + b), abs(m) * summation_bound(k * k, mag) + blend_bound(a, b)


# --- lnx_aug_affine -----------------------------------------------------------------------------------------------------------------
def affine_gather(x, m6):
    """x [planes, H, W], m6 = the output -> source matrix the kernel is given.  The direct definition in float64:
    y[h, w] = x[rint(sy), rint(sx)] (round half to even), zero outside, (sx, sy) = M (w - cx, h - cy) + (cx, cy), then the clamp.
    Returns (y fp32, sx float64 [H, W], sy float64 [H, W]) with the unrounded source coordinates."""
    P, H, W = x.shape
    m = [f32(v) for v in m6]
    cx, cy = 0.5 * (W - 1), 0.5 * (H - 1)
    dy, dx = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=x.device) - cy, torch.arange(W, dtype=torch.float64, device=x.device) - cx, indexing="ij")
    sx = m[0] * dx + m[1] * dy + m[2] + cx
    sy = m[3] * dx + m[4] * dy + m[5] + cy
    ix, iy = torch.round(sx).long(), torch.round(sy).long()
    inside = (ix >= 0) & (ix <= W - 1) & (iy >= 0) & (iy <= H - 1)
    y = torch.where(inside, x[:, iy.clamp(0, H - 1), ix.clamp(0, W - 1)], torch.zeros((), dtype=x.dtype, device=x.device))
    return A.clamp01(y), sx, sy


def near_tie(sx, sy, band=BAND):
    """Pixels whose source coordinate lies within `band` of k + 0.5 in x or y: there fp32 and the normalised-grid arithmetic of
    aug_oracle.affine may legitimately round to different neighbours."""
    def frac(v):
        return (v - torch.floor(v) - 0.5).abs()
    return (frac(sx) <= band) | (frac(sy) <= band)


# --- lnx_erase_rects ----------------------------------------------------------------------------------------------------------------
def erase(x, rects, vals):
    """x [B, C, H, W], rects: rows of (image, y0, x0, h, w), vals [n, C] -> x with x[image, c, y0:y0+h, x0:x0+w] = vals[j, c], in list
    order.  include/lnx.h: a rectangle of an image outside [0, B) or with h <= 0 or w <= 0 is skipped, the rest is clipped."""
    out = x.clone()
    B, _, H, W = x.shape
    for j, (b, y0, x0, h, w) in enumerate(torch.as_tensor(rects).tolist()):
        if b < 0 or b >= B or h <= 0 or w <= 0:
            continue
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        if ya < yb and xa < xb:
            out[b, :, ya:yb, xa:xb] = vals[j][:, None, None]
    return out


def pixel_values(x, noise):
    """GPURandomErasing's 'pixel' value, noise std + mean per (sample, channel) of x [B, C, H, W] -> (float64 [B, C], bound), before
    the clamp.  mean: a sum of n = H W terms over n.  std = sqrt(ss / (n - 1)), ss = sum (x - mean)^2: three roundings inside a
    term (hence n + 1 for summation_bound's n), the mean's own error enters ss only as n mean_b^2 (the first-order term vanishes at
    the true mean); a quotient and a root add one u each.  The final noise std + mean is one fma_bound."""
    n = x.shape[2] * x.shape[3]
    x64 = x.double()
    mean = x64.mean((2, 3))
    mean_b = summation_bound(n, x64.abs().sum((2, 3))) / n
    ss = ((x64 - mean[:, :, None, None]) ** 2).sum((2, 3))
    std = (ss / (n - 1)).sqrt()
    std_b = (summation_bound(n + 1, ss) + n * mean_b ** 2) / (n - 1) / (2 * std) + 2 * U * std
    t = noise.double() * std
    return t + mean, noise.double().abs() * std_b + mean_b + fma_bound(t, mean)


# --- lnx_u8hwc_to_f32chw ------------------------------------------------------------------------------------------------------------
def u8_to_f32(raw):
    """uint8 [B, H, W, C] -> fp32 [B, C, H, W]: permute(0, 3, 1, 2).float() / 255, the quotient correctly rounded."""
    f = raw.permute(0, 3, 1, 2).float().contiguous()
    return f / _s(255.0, f)


# --- lnx_mix_meta -------------------------------------------------------------------------------------------------------------------
def mix_meta(aux, masks, perm, pick, bounds):
    """(out_aux, out_mask) of the chunk-wise hard pick: oracle/mformer_oracle._mix_meta_chunks.  Columns outside every chunk come
    out as zero / false."""
    return _mix_meta_chunks(aux, masks, perm, pick, [tuple(b) for b in bounds])
