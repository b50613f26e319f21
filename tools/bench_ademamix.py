"""FusedAdEMAMix.step() against FusedAdamW.step() and against an eager per-parameter AdEMAMix loop (the op sequence of
linnaeus/optimizers/ademamix.py: what a linnaeus user with OPTIMIZER.NAME = ademamix runs today), on the parameter lists
of mFormerV1_sm (four Linear heads, 224) and mFormerV1_xl as built by linnaeus_amd.

    python tools/bench_ademamix.py [--steps 20] [--warmup 5] [--arch sm,xl]

Times with device events after warm-up; reports us per step and the HBM rate at 36 bytes per parameter (AdEMAMix: read
p, g, m1, v, m3, write p, m1, v, m3) or 28 (AdamW).  The eager loop's rate is the same byte count over its time (it
moves many more bytes).  Last line: one JSON object with every number.
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linnaeus_amd.optim import FusedAdamW, FusedAdEMAMix, ademamix_schedule  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
HYPER = dict(lr=1e-4, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0.05, alpha=5.0, T_alpha_beta3=1000)


def shapes_of(arch):
    from linnaeus_amd import arch_config, build_model

    cfg = arch_config(arch, 224)
    cfg.DATA.TASK_KEYS_H5 = [t for t, _ in TASKS]
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in TASKS}
    model = build_model(cfg, num_classes={t: c for t, c in TASKS})
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


class EagerAdEMAMix:
    """per-parameter loop, 13 tensor ops each, as the reference issues them"""

    def __init__(self, params, lr, betas, eps, weight_decay, alpha, T_alpha_beta3):
        self.params, self.lr, self.betas, self.eps, self.wd, self.alpha, self.T = params, lr, betas, eps, weight_decay, alpha, T_alpha_beta3
        self.state = [(torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)) for p in params]
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        b1, b2, b3 = self.betas
        lr, t = self.lr, self.t
        alpha_t, b3t = ademamix_schedule(t, self.alpha, b1, b3, self.T)
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        for p, (m, v, s) in zip(self.params, self.state):
            g = p.grad
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            s.mul_(b3t).add_(g, alpha=1 - b3t)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(self.eps)
            if self.wd != 0:
                p.add_(p, alpha=-self.wd * lr)
            p.addcdiv_(m + alpha_t * s, denom, value=-lr / bc1)


def timed(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps * 1e3  # us per step


def run(arch, steps, warmup):
    shapes = shapes_of(arch)
    n = sum(math.prod(s) for s in shapes)
    print(f"[{arch}] {n / 1e6:.2f} M parameters in {len(shapes)} tensors", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(*s, device="cuda", generator=gen) * 0.02) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
    res = {"params": n, "tensors": len(shapes)}
    cases = [
        ("fused_adamw", 28, lambda: FusedAdamW(params, lr=HYPER["lr"], betas=HYPER["betas"][:2], eps=HYPER["eps"], weight_decay=HYPER["weight_decay"])),
        ("fused_adamw_clip", 28, lambda: FusedAdamW(params, lr=HYPER["lr"], betas=HYPER["betas"][:2], eps=HYPER["eps"], weight_decay=HYPER["weight_decay"],
                                                    max_grad_norm=1.0)),
        ("fused_ademamix", 36, lambda: FusedAdEMAMix(params, **HYPER)),
        ("fused_ademamix_clip", 36, lambda: FusedAdEMAMix(params, max_grad_norm=1.0, **HYPER)),
        ("eager_ademamix", 36, lambda: EagerAdEMAMix(params, **HYPER)),
    ]
    for name, bpp, make in cases:
        opt = make()
        us = timed(opt.step, steps, warmup)
        res[name + "_us"] = round(us, 1)
        print(f"[{arch}] {name:20s} {us:10.1f} us/step  {n * bpp / (us * 1e-6) / 1e12:5.2f} TB/s ({bpp} bytes per parameter)", flush=True)
        del opt
        torch.cuda.empty_cache()
    # the eager loop with the clip linnaeus applies before it (train.py: clip_grad_norm_, then optimizer.step)
    opt = EagerAdEMAMix(params, **HYPER)

    def eager_clip():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()

    us = timed(eager_clip, steps, warmup)
    res["eager_ademamix_clip_us"] = round(us, 1)
    print(f"[{arch}] {'eager_ademamix_clip':20s} {us:10.1f} us/step  (clip_grad_norm_, then the loop)", flush=True)
    res["ademamix_over_adamw"] = round(res["fused_ademamix_us"] / res["fused_adamw_us"], 3)
    res["eager_over_fused"] = round(res["eager_ademamix_us"] / res["fused_ademamix_us"], 1)
    print(f"[{arch}] fused AdEMAMix / fused AdamW {res['ademamix_over_adamw']:.3f}x (bytes 36/28 = 1.286x);  eager / fused AdEMAMix {res['eager_over_fused']:.1f}x",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arch", default="sm,xl")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    for arch in args.arch.split(","):
        out[arch] = run(arch, args.steps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
