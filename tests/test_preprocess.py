"""lnx_preprocess / DevicePreprocessor without a GPU: the numpy restatement against Pillow itself and against the recorded fixture, the
library's host coefficient builder against the restatement's tables, the ctypes mirrors against the C compiler, and every refusal
the launcher and the Python class make on the host.  Everything is compared by exact equality."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from linnaeus_amd import DevicePreprocessor
from linnaeus_amd import _lib as L
from tests import preprocess_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "preprocess.npz")
ALL = [(src, dst, content) for src, dst in R.CASES for content in R.CONTENTS]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_against_fixture(g, got_u8, src, dst, content, fname):
    """got_u8 [H, W, 3] against what the fixture holds of Pillow's result: the whole image, or its SHA-256 and three bands of rows."""
    name = R.case_name(src, dst, content)
    if f"u8_{name}_{fname}" in g.files:
        want = g[f"u8_{name}_{fname}"]
        assert got_u8.shape == want.shape and np.array_equal(got_u8, want), (name, fname, np.argwhere(got_u8 != want)[:4].tolist())
    else:
        assert np.array_equal(R.bands(got_u8), g[f"rows_{name}_{fname}"]), (name, fname, "bands")
        assert np.array_equal(R.digest(got_u8), g[f"sha_{name}_{fname}"]), (name, fname, "digest")


def test_restatement_equals_pillow_bit_for_bit():
    Image = pytest.importorskip("PIL.Image")
    pil = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}
    for src, dst, content in ALL:
        img = R.pattern(*src, content)
        for fname, code in R.FILTERS.items():
            want = np.array(Image.fromarray(img, "RGB").resize((dst[1], dst[0]), pil[fname]))
            assert np.array_equal(R.resize(img, dst[0], dst[1], code), want), (src, dst, content, fname)


def test_restatement_equals_the_fixture():
    g = np.load(GOLDEN)
    mean, std = g["mean"], g["std"]
    for src, dst, content in ALL:
        name = R.case_name(src, dst, content)
        img = R.pattern(*src, content)
        if (src, dst) not in R.LARGE:
            assert np.array_equal(img, g[f"src_{name}"]), name
        for fname, code in R.FILTERS.items():
            u8 = R.resize(img, dst[0], dst[1], code)
            check_against_fixture(g, u8, src, dst, content, fname)
            if (src, dst) not in R.LARGE:
                assert np.array_equal(bits(R.normalize(u8, mean, std)), bits(g[f"f32_{name}_{fname}"])), (name, fname)
    every = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert np.array_equal(bits(R.normalize(every, mean, std)[:, 0, :]), bits(g["bytes_f32"]))
    assert len({float(v) for v in mean}) == 3 and len({float(v) for v in std}) == 3  # a channel mix-up cannot pass


def test_checkerboards_reach_both_clamps():
    """Bicubic on the enlarged 0 / 255 checkerboards overshoots: some sums leave [0, 255] before the clamp, on both sides."""
    for (h, w), (_, W) in (((7, 5), (16, 16)), ((33, 47), (224, 224))):
        img = R.pattern(h, w, "checker").astype(np.int64)
        k, b = R.coeffs(w, W, R.BICUBIC)
        sums = np.stack([(k[x, : b[x, 1]][None, :, None] * img[:, b[x, 0]: b[x, 0] + b[x, 1]]).sum(1) + (1 << 21) for x in range(W)]) >> 22
        assert sums.min() < 0 and sums.max() > 255, (h, w)


PAIRS = [(i, o) for i in range(1, 49) for o in range(1, 49)] + [(4000, 224), (224, 4000), (16384, 1)]


def test_host_coefficient_builder_equals_the_restatement():
    lib = L.lib()
    assert lib.lnx_version() >= 106
    for i, o in PAIRS:
        for code in (R.NEAREST, R.BILINEAR, R.BICUBIC):
            taps = lib.lnx_resize_taps(i, o, code)
            assert taps == R.taps(i, o, code), (i, o, code)
            k = np.full(o * taps + 8, -7, np.int32)  # eight guard entries behind each table
            b = np.full(o * (1 if code == R.NEAREST else 2) + 8, -7, np.int32)
            assert lib.lnx_resize_coeffs(i, o, code, None if code == R.NEAREST else k.ctypes.data, b.ctypes.data) == 0, lib.lnx_last_error()
            rk, rb = R.coeffs(i, o, code)
            assert (k[-8:] == -7).all() and (b[-8:] == -7).all(), (i, o, code)
            assert np.array_equal(b[:-8], rb.reshape(-1)), (i, o, code)
            if code != R.NEAREST:
                assert np.array_equal(k[:-8].reshape(o, taps), rk), (i, o, code)
    assert lib.lnx_resize_taps(1000, 7, R.BICUBIC) == 573 and lib.lnx_resize_taps(1000, 7, R.BILINEAR) == 287
    assert lib.lnx_resize_taps(0, 4, R.BILINEAR) == 0 and b"lnx_resize_taps" in lib.lnx_last_error()
    assert lib.lnx_resize_taps(4, 4, 3) == 0
    assert lib.lnx_resize_coeffs(4, 16385, R.BILINEAR, k.ctypes.data, b.ctypes.data) != 0 and b"lnx_resize_coeffs" in lib.lnx_last_error()


def test_ctypes_mirrors_have_the_sizes_the_c_compiler_gives(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"lnx_preprocess_image": L.PreprocessImage, "lnx_preprocess_args": L.PreprocessArgs}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) +
                   '    printf("out %zu\\n", offsetof(lnx_preprocess_args, out));\n    printf("rows %zu\\n", offsetof(lnx_preprocess_image, rows));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in pairs.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    assert int(got["out"]) == L.PreprocessArgs.out.offset and int(got["rows"]) == L.PreprocessImage.rows.offset
    assert (L.RESIZE_NEAREST, L.RESIZE_BILINEAR, L.RESIZE_BICUBIC, L.PREPROCESS_MAX_SIDE) == (0, 1, 2, 16384)


def good_args(h=40, w=50, H=16, W=24, code=R.BILINEAR):
    """A batch of one image that passes every check (the pointers are fake and never dereferenced: nothing must be launched)."""
    lib = L.lib()
    images = (L.PreprocessImage * 1)()
    d = images[0]
    d.h, d.w = h, w
    d.hk, d.hb, d.vk, d.vb, d.src = 128, 4096, 8192, 12288, 16384
    scratch = lib.lnx_preprocess_scratch_bytes(images, 1, H, W, code)
    assert scratch >= 0, lib.lnx_last_error()
    a = L.PreprocessArgs()
    a.n, a.H, a.W, a.filter = 1, H, W, code
    a.images = images
    a.blob, a.blob_bytes, a.images_off = 0x10000, 16384 + h * w * 3, 0
    a.scratch, a.scratch_bytes = 0x20000, scratch
    a.mean[:] = [0.5, 0.5, 0.5]
    a.std[:] = [0.25, 0.25, 0.25]
    a.out = 0x30000
    return a, images


def refused(a, needle):
    lib = L.lib()
    assert lib.lnx_preprocess(C.byref(a), None) != 0, needle
    assert needle in lib.lnx_last_error(), (needle, lib.lnx_last_error())


def test_every_refusal_of_the_launcher():
    lib = L.lib()
    assert lib.lnx_preprocess(None, None) != 0 and b"NULL arguments" in lib.lnx_last_error()
    a, keep = good_args()
    assert keep[0].htaps == R.taps(50, 24, R.BILINEAR) and keep[0].vtaps == R.taps(40, 16, R.BILINEAR)
    _, vb = R.coeffs(40, 16, R.BILINEAR)
    assert (keep[0].y0, keep[0].rows) == (vb[0, 0], vb[-1, 0] + vb[-1, 1] - vb[0, 0])
    assert a.scratch_bytes == -(-keep[0].rows * 24 * 3 // 16) * 16
    for field in ("images", "blob", "out"):
        a, keep = good_args()
        setattr(a, field, None)
        refused(a, b"NULL pointer")
    a, keep = good_args()
    a.scratch = None
    refused(a, b"NULL scratch")
    for n in (0, -3):
        a, keep = good_args()
        a.n = n
        refused(a, b"n=")
    for H, W in ((0, 24), (16, -1), (16, 16385)):
        a, keep = good_args()
        a.H, a.W = H, W
        refused(a, b"output side")
    for h, w in ((0, 50), (40, 16385), (-2, 50)):
        a, keep = good_args()
        keep[0].h, keep[0].w = h, w
        refused(a, b"source side")
    for code in (-1, 3, 7):
        a, keep = good_args()
        a.filter = code
        refused(a, b"unknown filter")
    for c in range(3):
        a, keep = good_args()
        a.std[c] = 0.0
        refused(a, f"std[{c}] == 0".encode())
    a, keep = good_args()
    a.scratch_bytes -= 1
    refused(a, b"scratch too small")
    a, keep = good_args()
    keep[0].scratch = 16
    refused(a, b"scratch too small")
    # what the kernels address with: derived fields that do not belong to (h, w), offsets that leave the blob, misaligned tables
    a, keep = good_args()
    keep[0].rows += 1
    refused(a, b"expected")
    a, keep = good_args()
    keep[0].y0 -= 1
    refused(a, b"expected")
    a, keep = good_args()
    a.blob_bytes -= 1
    refused(a, b"source at")
    a, keep = good_args()
    keep[0].hk = 2
    refused(a, b"horizontal tables")
    a, keep = good_args()
    keep[0].vb = a.blob_bytes - 4
    refused(a, b"vertical tables")
    a, keep = good_args()
    a.images_off = a.blob_bytes - 8
    refused(a, b"descriptor table")
    a, keep = good_args()
    a.blob = 0x10008
    refused(a, b"16-byte aligned")
    a, keep = good_args(code=R.NEAREST)
    assert a.scratch_bytes == 0
    keep[0].hb = -4
    refused(a, b"index tables")
    # the sizing entry point refuses the same things by name
    images = (L.PreprocessImage * 1)()
    images[0].h, images[0].w = 40, 50
    assert lib.lnx_preprocess_scratch_bytes(None, 1, 16, 24, 1) < 0 and b"NULL images" in lib.lnx_last_error()
    assert lib.lnx_preprocess_scratch_bytes(images, 0, 16, 24, 1) < 0 and b"n=0" in lib.lnx_last_error()
    assert lib.lnx_preprocess_scratch_bytes(images, 1, 0, 24, 1) < 0 and b"output side" in lib.lnx_last_error()
    assert lib.lnx_preprocess_scratch_bytes(images, 1, 16, 24, 5) < 0 and b"unknown filter" in lib.lnx_last_error()
    images[0].w = 16385
    assert lib.lnx_preprocess_scratch_bytes(images, 1, 16, 24, 1) < 0 and b"source side" in lib.lnx_last_error()
    # nothing to do on either axis: no scratch, no taps
    images[0].h, images[0].w = 16, 24
    assert lib.lnx_preprocess_scratch_bytes(images, 1, 16, 24, 2) == 0 and (images[0].htaps, images[0].vtaps, images[0].rows) == (0, 0, 16)
    images[0].h, images[0].w = 40, 24  # vertical only: read in place
    assert lib.lnx_preprocess_scratch_bytes(images, 1, 16, 24, 2) == 0 and images[0].vtaps == R.taps(40, 16, R.BICUBIC)


def test_python_level_refusals():
    import torch

    with pytest.raises(L.LnxError, match="unknown interpolation 'lanczos'"):
        DevicePreprocessor(interpolation="lanczos")
    with pytest.raises(L.LnxError, match="image_size"):
        DevicePreprocessor(image_size=(1, 224, 224))
    with pytest.raises(L.LnxError, match="no zero std"):
        DevicePreprocessor(std=(0.2, 0.0, 0.2))
    pre = DevicePreprocessor.from_input_config({"image_size": [3, 16, 24], "image_mean": [0.1, 0.2, 0.3], "image_std": [0.5, 0.6, 0.7],
                                                "image_interpolation": "NEAREST_EXACT"})
    assert (pre.H, pre.W, pre.filter, pre.mean, pre.std) == (16, 24, L.RESIZE_NEAREST, [0.1, 0.2, 0.3], [0.5, 0.6, 0.7])
    for bad in (np.zeros((4, 5, 4), np.uint8), np.zeros((4, 5), np.uint8), torch.zeros(4, 5, 1, dtype=torch.uint8)):
        with pytest.raises(L.LnxError, match="three channels"):
            pre([np.zeros((4, 5, 3), np.uint8), bad])
    with pytest.raises(L.LnxError, match="expected uint8"):
        pre([np.zeros((4, 5, 3), np.float32)])
    with pytest.raises(TypeError, match="Unsupported image type"):
        pre(["a path"])
    if not torch.cuda.is_available():
        with pytest.raises(L.LnxError, match="needs a HIP device: linnaeus_amd has no CPU fallback"):
            pre([np.zeros((4, 5, 3), np.uint8)])
