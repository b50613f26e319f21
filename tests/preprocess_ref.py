"""Plain numpy restatement of lnx_preprocess: what the reference's preprocess_image_batch (linnaeus/inference/preprocessing.py:29-82)
does per image with TF.resize of a PIL image (Pillow's Image.resize on 8-bit RGB), TF.to_tensor and TF.normalize, in Pillow's own
arithmetic, so that the result is Pillow's bit for bit.

  bilinear / bicubic   two separable passes in 22-bit fixed point with a uint8 rounding between them (Pillow's Resample.c).  Per axis
                       inS -> outS, all in double:  scale = inS / outS, fs = max(scale, 1), support = S * fs (S = 1 / 2),
                       taps = 2 * ceil(support) + 1;  per output xx: center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0),
                       xmax = min(int(center + support + 0.5), inS), n = xmax - xmin;  w[x] = f((x + xmin - center + 0.5) * (1 / fs)),
                       summed in order and divided by the sum when that is not 0;  k[x] = int(w * 2^22 +- 0.5) towards the sign of w.
                       A pass: out = clamp((2^21 + sum_x src[xmin + x] * k[x]) >> 22, 0, 255).  Horizontal first, only if the width
                       changes, then vertical, only if the height changes.
  nearest              per axis a = inS / outS, xo = a * 0.5; per output in turn: index = min(int(xo), inS - 1), xo += a.
  to_tensor/normalize  fp32: (u8 / 255 - mean[c]) / std[c], mean and std rounded to fp32 first, both divisions correctly rounded.
"""
import math

import numpy as np

NEAREST, BILINEAR, BICUBIC = 0, 1, 2
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR, "bicubic": BICUBIC}
PRECISION_BITS = 22


def _bilinear(t):
    t = np.abs(t)
    return np.where(t < 1.0, 1.0 - t, 0.0)


def _bicubic(t):
    a = -0.5
    t = np.abs(t)
    with np.errstate(over="ignore"):
        inner = ((a + 2.0) * t - (a + 3.0)) * t * t + 1
        outer = (((t - 5) * t + 8) * t - 4) * a
    return np.where(t < 1.0, inner, np.where(t < 2.0, outer, 0.0))


def taps(in_size, out_size, filt):
    """Row stride of the coefficient table: Pillow's ksize; 1 for nearest."""
    if filt == NEAREST:
        return 1
    fs = max(in_size / out_size, 1.0)
    return int(math.ceil((1.0 if filt == BILINEAR else 2.0) * fs)) * 2 + 1


def coeffs(in_size, out_size, filt):
    """-> (k int32 [out, taps], zero beyond n; bounds int32 [out, 2] = (xmin, n)).  Nearest: (None, index int32 [out])."""
    if filt == NEAREST:
        a = in_size / out_size
        xo = a * 0.5
        idx = np.empty(out_size, np.int32)
        for xx in range(out_size):
            idx[xx] = min(int(xo), in_size - 1)
            xo += a
        return None, idx
    f = _bilinear if filt == BILINEAR else _bicubic
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = (1.0 if filt == BILINEAR else 2.0) * fs
    ss = 1.0 / fs
    kt = taps(in_size, out_size, filt)
    k = np.zeros((out_size, kt), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w = f((np.arange(n, dtype=np.float64) + xmin - center + 0.5) * ss)
        ww = 0.0
        for v in w:  # summed in order
            ww += float(v)
        if ww != 0.0:
            w = w / ww
        scaled = w * float(1 << PRECISION_BITS)
        k[xx, :n] = np.where(w < 0, np.trunc(scaled - 0.5), np.trunc(scaled + 0.5)).astype(np.int64)
        bounds[xx] = (xmin, n)
    return k, bounds


def _pass(src, k, bounds):
    """Resample axis 0 of src uint8 [in, ...] -> uint8 [out, ...]."""
    out = np.empty((k.shape[0],) + src.shape[1:], np.uint8)
    s = src.astype(np.int64)
    for xx in range(k.shape[0]):
        xmin, n = bounds[xx]
        acc = np.tensordot(k[xx, :n].astype(np.int64), s[xmin: xmin + n], axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31  # Pillow accumulates in int
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img, H, W, filt):
    """img uint8 [h, w, 3] -> uint8 [H, W, 3], Pillow's Image.resize((W, H), filt)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    if filt == NEAREST:
        return img[coeffs(h, H, filt)[1].astype(np.int64)][:, coeffs(w, W, filt)[1].astype(np.int64)]
    out = img
    if W != w:
        k, b = coeffs(w, W, filt)
        out = _pass(out.transpose(1, 0, 2), k, b).transpose(1, 0, 2)
    if H != h:
        k, b = coeffs(h, H, filt)
        out = _pass(out, k, b)
    return np.ascontiguousarray(out)


def normalize(u8, mean, std):
    """uint8 [H, W, 3] -> fp32 [3, H, W]: TF.to_tensor then TF.normalize."""
    mean = np.asarray(mean, np.float32).reshape(3, 1, 1)
    std = np.asarray(std, np.float32).reshape(3, 1, 1)
    v = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return ((v - mean) / std).astype(np.float32)


def preprocess(images, H, W, filt, mean, std):
    """list of uint8 [h, w, 3] -> fp32 [N, 3, H, W]."""
    if not images:
        return np.empty((0, 3, H, W), np.float32)
    return np.stack([normalize(resize(im, H, W, filt), mean, std) for im in images])


# the cases of tests/golden/preprocess.npz: source (h, w) -> target (H, W)
CASES = [((7, 5), (16, 16)), ((1, 1), (4, 4)), ((1, 9), (3, 3)), ((16, 16), (16, 16)), ((16, 40), (16, 16)), ((40, 16), (16, 16)),
         ((37, 53), (16, 24)), ((301, 17), (8, 8)), ((3, 1000), (5, 7)), ((33, 47), (224, 224)), ((375, 500), (224, 224)),
         ((480, 640), (384, 384))]
LARGE = {((33, 47), (224, 224)), ((375, 500), (224, 224)), ((480, 640), (384, 384))}  # the real target sizes: recorded as uint8 only
CONTENTS = ("noise", "checker")
BAND = 4  # rows of the three bands (top, middle, bottom) kept beside the digest of a large noise result


def bands(u8):
    """The rows of a large result that the fixture keeps in full beside its SHA-256 (resampled noise does not compress)."""
    H = u8.shape[0]
    return np.concatenate([u8[:BAND], u8[H // 2: H // 2 + BAND], u8[H - BAND:]])


def digest(u8):
    import hashlib

    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(u8).tobytes()).digest(), np.uint8)


def pattern(h, w, content):
    """Closed-form integer content: "noise" = a multiplicative hash of (y, x, c), "checker" = 0 / 255 squares of one pixel."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64), np.arange(3, dtype=np.uint64), indexing="ij")
    if content == "checker":
        return (((y + x) & np.uint64(1)) * np.uint64(255)).astype(np.uint8)
    v = (y * np.uint64(73856093)) ^ (x * np.uint64(19349663)) ^ (c * np.uint64(83492791))
    v = (v * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return ((v >> np.uint64(13)) & np.uint64(255)).astype(np.uint8)


def case_name(src, dst, content):
    return f"{src[0]}x{src[1]}_{dst[0]}x{dst[1]}_{content}"
