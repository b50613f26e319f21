#!/usr/bin/env python3
"""What image preprocessing costs in front of the eval forward of mFormerV1_sm (bf16, 224 px, bilinear).

Two batches: `uniform` = 64 images of 500 x 375 (w x h), `mixed` = 64 images of eight different sizes from 160 x 120 to 1024 x 768.
Per batch, legs in ONE process, warm-up calls then timed calls between two device synchronisations, alternated `--repeats` times so
that drift hits all of them alike; medians are reported:

  a    the reference's recipe restated (inference/preprocessing.py:29-82): per image PIL Image.resize, to_tensor, normalize (written
       out in torch CPU fp32: torchvision is not needed), torch.stack, .cuda()
  b    DevicePreprocessor alone (one pinned copy, at most two launches)
  fwd  the sm eval forward alone on a resident batch of the same size
  a+f  leg a, then the forward on its result;  b+f  leg b, then the forward on its result

Before any timing the tool asserts that legs a and b give the same bits.  --kernel-only runs leg b alone, for a kernel trace of its
own.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
MIXED = [(120, 160), (240, 320), (375, 500), (480, 640), (600, 800), (768, 1024), (333, 500), (500, 333)]  # (h, w)


def make_batch(kind, n, seed):
    rng = np.random.default_rng(seed)
    sizes = [(375, 500)] * n if kind == "uniform" else [MIXED[i % len(MIXED)] for i in range(n)]
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


def reference_recipe(pils, H, W, code):
    """preprocess_image_batch, with TF.to_tensor / TF.normalize written out (torchvision/transforms/functional.py)."""
    mean = torch.as_tensor(MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=torch.float32).view(-1, 1, 1)
    out = []
    for im in pils:
        u8 = np.array(im.resize((W, H), code))
        t = torch.from_numpy(u8).permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)
        out.append(t.sub_(mean).div_(std))
    return torch.stack(out)


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--iters-a", type=int, default=5, help="timed calls of the reference recipe (slow)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--no-forward", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_preprocess.py needs the MI355X: timings taken elsewhere say nothing")
    from PIL import Image

    from linnaeus_amd import DevicePreprocessor, arch_config, build_model

    H = W = args.size
    pre = DevicePreprocessor((3, H, W), MEAN, STD, "bilinear")
    batches = {kind: make_batch(kind, args.images, 7 + i) for i, kind in enumerate(("uniform", "mixed"))}
    pils = {kind: [Image.fromarray(a, "RGB") for a in b] for kind, b in batches.items()}
    for kind, b in batches.items():
        want = reference_recipe(pils[kind], H, W, Image.BILINEAR)
        got = pre(b).cpu()
        assert got.numpy().tobytes() == want.numpy().tobytes(), f"{kind}: DevicePreprocessor differs from the reference recipe"
    print(f"[bench_preprocess] legs a and b agree bit for bit on both batches ({args.images} images -> {H} x {W})")
    if args.kernel_only:
        for kind, b in batches.items():
            print(f"{kind}: {timed(lambda: pre(b), args.warmup, args.iters):.3f} ms per call")
        return
    model = None
    if not args.no_forward:
        heads = {"taxa_L10": 1000, "taxa_L20": 300, "taxa_L30": 80, "taxa_L40": 20}
        cfg = arch_config("sm", args.size)
        model = build_model(cfg, num_classes=heads).cuda().eval()
        model.set_compute_dtype("bf16")
        meta_width = sum(model.meta_dims)
    result = {"images": args.images, "size": args.size, "warmup": args.warmup, "iters": args.iters, "iters_a": args.iters_a, "repeats": args.repeats}
    for kind, b in batches.items():
        pl = pils[kind]
        x_res = pre(b).clone()
        aux = torch.rand(len(b), meta_width, device="cuda") if model is not None and meta_width else None

        def fwd(x):
            with torch.no_grad():
                return model(x, aux)

        legs = {"a": (lambda: reference_recipe(pl, H, W, Image.BILINEAR).cuda(), args.iters_a), "b": (lambda: pre(b), args.iters)}
        if model is not None:
            legs["fwd"] = (lambda: fwd(x_res), args.iters)
            legs["a+f"] = (lambda: fwd(reference_recipe(pl, H, W, Image.BILINEAR).cuda()), args.iters_a)
            legs["b+f"] = (lambda: fwd(pre(b)), args.iters)
        times = {k: [] for k in legs}
        for _ in range(args.repeats):
            for k, (fn, iters) in legs.items():
                times[k].append(timed(fn, min(args.warmup, iters), iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        src_mb = sum(a.nbytes for a in b) / 1e6
        print(f"{kind}: {src_mb:.1f} MB of sources -> {len(b) * 3 * H * W * 4 / 1e6:.1f} MB fp32; ms per batch (median of {args.repeats}; all runs): " +
              "; ".join(f"{k} {med[k]:.3f} ({', '.join(f'{t:.3f}' for t in times[k])})" for k in legs))
        result[kind] = {"source_mb": round(src_mb, 2), **{k: round(v, 4) for k, v in med.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
