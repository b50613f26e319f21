#!/usr/bin/env python3
"""Generate tests/golden/preprocess.npz: what the reference's preprocess_single_image (linnaeus/inference/preprocessing.py:29-55)
computes, recorded from the libraries it calls.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_preprocess.py

TF.resize of a PIL image is PIL's Image.resize (torchvision/transforms/_functional_pil.py: `img.resize(tuple(size[::-1]), interpolation)`),
called here directly.  torchvision is not installed, so TF.to_tensor and TF.normalize are written out in torch CPU fp32 as torchvision has
them (transforms/functional.py, to_tensor: `img.permute((2, 0, 1)).contiguous()` then `.to(dtype=torch.float32).div(255)`;
transforms/_functional_tensor.py, normalize: `mean = torch.as_tensor(mean, dtype=tensor.dtype)`, likewise std, both viewed as [-1, 1, 1],
then `tensor.sub_(mean).div_(std)`).  Writes numbers only:

  cases     tests/preprocess_ref.py CASES x CONTENTS (closed-form integer patterns, rebuilt by the tests) x the three filters:
            `u8_<case>_<filter>` = PIL's uint8 [H, W, 3]; for the small cases also `f32_<case>_<filter>` = the fp32 [3, H, W] after
            to_tensor / normalize with `mean` / `std`, and `src_<case>` = the source.  The noise results at the three real target sizes
            do not compress (2 MB), so of those the file keeps `sha_<case>_<filter>` = the SHA-256 of PIL's bytes and
            `rows_<case>_<filter>` = three bands of rows (preprocess_ref.bands); their checkerboard twins are kept whole
  bytes     `bytes_f32` [3, 256]: to_tensor / normalize of every byte value in every channel
"""
import os
import sys

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from tests import preprocess_ref as R  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
PIL_FILTER = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}


def to_tensor_normalize(u8):
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)
    mean = torch.as_tensor(MEAN, dtype=t.dtype).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=t.dtype).view(-1, 1, 1)
    return t.sub_(mean).div_(std).numpy()


out = {"mean": np.asarray(MEAN, np.float64), "std": np.asarray(STD, np.float64)}
for src, dst in R.CASES:
    for content in R.CONTENTS:
        name = R.case_name(src, dst, content)
        img = R.pattern(*src, content)
        small = (src, dst) not in R.LARGE
        if small:
            out[f"src_{name}"] = img
        for fname, code in PIL_FILTER.items():
            u8 = np.array(Image.fromarray(img, "RGB").resize((dst[1], dst[0]), code))
            if small or content == "checker":
                out[f"u8_{name}_{fname}"] = u8
            else:
                out[f"sha_{name}_{fname}"] = R.digest(u8)
                out[f"rows_{name}_{fname}"] = R.bands(u8)
            if small:
                out[f"f32_{name}_{fname}"] = to_tensor_normalize(u8)
out["bytes_f32"] = to_tensor_normalize(np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2))[:, 0, :]
path = os.path.join(REPO, "tests", "golden", "preprocess.npz")
np.savez_compressed(path, **out)
print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes, Pillow {Image.__version__}, torch {torch.__version__}")
