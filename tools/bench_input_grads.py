"""What input gradients cost: the stem's data-gradient kernel against its two-launch fallback, and a training step with and without
`images.requires_grad`.

    python tools/bench_input_grads.py [--batch 256] [--steps 10] [--warmup 5] [--repeats 7] [--log profiles/input_grad_bench.log]

(a) Kernel.  `lnx_stem_dgrad` at the sm stem (M0 = batch * 56 * 56 patches, Cout = 96, Cin = 3, bf16) against the composition the plan
    runs for geometries the kernel does not carry: `lnx_gemm_nt` on the transposed weight copy (fp32 [M0, 48] out) + `lnx_col2im_stem`.
    Microseconds per call and GB/s on the bytes the operation must move (dY read once: M0 * Cout * 2, dx written once: batch * 3 * 224 *
    224 * 4; 308 MB at batch 256).  The legs alternate round by round; median [min .. max] of the rounds.
(b) Step.  mFormerV1_sm bf16, forward + probe loss + backward in direct gradient mode, with the images as a plain tensor and as a
    leaf that requires grad (same model, same build, one plan each), alternated round by round; milliseconds per step.

Last line: one JSON object; the log file gets the same text.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps  # milliseconds per call


def alternate(legs, warmup, steps, repeats):
    for fn in legs.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            rounds[k].append(window(fn, steps))
    return {k: {"median": statistics.median(r), "min": min(r), "max": max(r)} for k, r in rounds.items()}


def kernel_legs(B):
    from linnaeus_amd import _lib as L
    from linnaeus_amd import ops

    Cin, H, W, Cout = 3, 224, 224, 96
    M0 = B * (H // 4) * (W // 4)
    g = torch.Generator(device="cuda").manual_seed(0)
    dy = torch.randn(M0, Cout, device="cuda", generator=g).to(torch.bfloat16)
    w = torch.zeros(Cout, 64, device="cuda")
    w[:, : Cin * 16] = torch.randn(Cout, Cin * 16, device="cuda", generator=g) / 7
    w = w.to(torch.bfloat16)
    wt = w[:, : Cin * 16].t().contiguous()
    dx = torch.empty(B, Cin, H, W, device="cuda")
    dx2 = torch.empty_like(dx)
    dcol = torch.empty(M0, Cin * 16, device="cuda")
    assert ops.stem_dgrad_ok(L.BF16, Cin, H, W, Cout)

    def fused():
        ops.stem_dgrad(dy, w, dx)

    def fallback():
        ops.gemm_nt(dy, wt, dcol)
        ops.col2im_stem(dcol, dx2)

    fused()
    fallback()
    torch.cuda.synchronize()
    diff = (dx - dx2).abs().max().item()
    return {"lnx_stem_dgrad": fused, "gemm_nt + col2im_stem": fallback}, M0 * Cout * 2 + dx.numel() * 4, M0, diff


def make_model():
    from linnaeus_amd import arch_config, build_model

    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = [t for t, _ in TASKS]
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in TASKS}
    torch.manual_seed(0)
    model = build_model(cfg, num_classes=dict(TASKS)).cuda().train()
    model.set_compute_dtype("bf16")
    model.grad_mode = "direct"
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    B = a.batch
    result = {"batch": B}
    legs, nbytes, M0, diff = kernel_legs(B)
    k = alternate(legs, a.warmup, 3 * a.steps, a.repeats)
    say(f"(a) stem data gradient, M0 = {M0}, Cout = 96, Cin = 3, bf16: {nbytes / 1e6:.0f} MB to move; max |fused - fallback| = {diff:.2e}")
    result["kernel"] = {"M0": M0, "bytes": nbytes, "max_abs_diff": diff}
    for name, r in k.items():
        us = {q: 1e3 * v for q, v in r.items()}
        gbs = nbytes / (r["median"] * 1e-3) / 1e9
        result["kernel"][name] = {"us": round(us["median"], 1), "min": round(us["min"], 1), "max": round(us["max"], 1), "GBps": round(gbs)}
        say(f"    {name:24s} {us['median']:8.1f} us [{us['min']:.1f} .. {us['max']:.1f}]  {gbs:6.0f} GB/s")
    del legs
    torch.cuda.empty_cache()

    model = make_model()
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    meta = torch.randn(B, sum(model.meta_dims), device="cuda", generator=g) if model.meta_dims else None

    def stepper(want_x):
        def step():
            xin = x.detach().requires_grad_(True) if want_x else x
            out = model(xin, meta)
            sum(v.float().square().mean() for v in out.values()).backward()
        return step

    s = alternate({"plain": stepper(False), "images.requires_grad": stepper(True)}, a.warmup, a.steps, a.repeats)
    say(f"(b) mFormerV1_sm bf16 batch {B}: forward + probe loss + backward, ms per step (median [min .. max] of {a.repeats} rounds of {a.steps} steps)")
    result["step"] = {}
    for name, r in s.items():
        result["step"][name] = {"ms": round(r["median"], 3), "min": round(r["min"], 3), "max": round(r["max"], 3)}
        say(f"    {name:24s} {r['median']:8.3f} ms [{r['min']:.3f} .. {r['max']:.3f}]")
    say(json.dumps(result))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
