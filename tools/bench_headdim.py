"""Attention head_dim 32 / 64 / 128 at equal width C: per-launch attention times and whole training steps.

    python tools/bench_headdim.py [--part ops|steps|all] [--steps 10] [--warmup 3]

  ops    lnx_attn_fwd / lnx_attn_bwd (bf16) at the mFormerV1_sm stage-3 / stage-4 shapes (C 384 / 768, B = 256) and the xl ones
         (C 1024 / 2048, B = 128), for the head counts that give head_dim 32, 64 and 128; us per call (the backward call is its two
         kernels + the freqs fold) and the ratio to head_dim 64.  Run it under `rocprofv3 --kernel-trace --stats` for per-kernel times.
  steps  one training step (bf16 forward + four-task cross entropy + backward, autograd grad mode, no optimizer) of sm at B = 256
         with NUM_HEADS [12, 24] / [6, 12] / [3, 6] and of xl at B = 128 with [32, 64] / [16, 32] / [8, 16]: ms per step.

Times are device-synchronised wall clock per call after warm-up.  Last line: one JSON object with every number.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linnaeus_amd import arch_config, build_model, ops  # noqa: E402
from linnaeus_amd.loss import multitask_cross_entropy  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
# (label, B, H, W, E, C): E = CLS + two metadata tokens, as the shipped configs at 224 px
OP_SHAPES = (("sm.s3", 256, 14, 14, 3, 384), ("sm.s4", 256, 7, 7, 3, 768), ("xl.s3", 128, 14, 14, 3, 1024), ("xl.s4", 128, 7, 7, 3, 2048))
STEP_CASES = (("sm", 256, ((12, 24), (6, 12), (3, 6))), ("xl", 128, ((32, 64), (16, 32), (8, 16))))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def bench_ops(a, res):
    for label, B, H, W, E, Cc in OP_SHAPES:
        N = H * W + E
        base = {}
        for hd in (64, 32, 128):
            heads = Cc // hd
            g = torch.Generator().manual_seed(hd)
            qkv = torch.randn(B * N, 3 * Cc, generator=g).cuda().bfloat16()
            freqs = torch.randn(2, heads, hd // 2, generator=g).cuda()
            dsin = torch.empty(2, H * W, heads, hd // 2, device="cuda")
            cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
            o = torch.empty(B * N, Cc, device="cuda", dtype=torch.bfloat16)
            lse = torch.empty(B, heads, N, device="cuda")
            do = torch.randn(B * N, Cc, generator=g).cuda().bfloat16()
            dqkv = torch.empty_like(qkv)
            delta = torch.empty_like(lse)
            dfreqs = torch.zeros(2, heads, hd // 2, device="cuda")
            tf = timed(lambda: ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads), a.op_steps, a.warmup)
            tb = timed(lambda: ops.attn_bwd(qkv, cos, o, lse, do, dqkv, delta, B, N, E, heads, dsin=dsin, dfreqs=dfreqs), a.op_steps, a.warmup)
            if hd == 64:
                base = {"fwd": tf, "bwd": tb}
            key = f"{label}.hd{hd}"
            res["ops"][key] = {"N": N, "heads": heads, "fwd_us": round(tf * 1e6, 1), "bwd_us": round(tb * 1e6, 1),
                               "fwd_x_hd64": round(tf / base["fwd"], 2), "bwd_x_hd64": round(tb / base["bwd"], 2)}
            print(f"{key:12s} N={N:3d} heads={heads:3d}  fwd {tf * 1e6:8.1f} us ({tf / base['fwd']:.2f}x hd64)   "
                  f"bwd {tb * 1e6:8.1f} us ({tb / base['bwd']:.2f}x hd64)", flush=True)


def bench_steps(a, res):
    for arch, B, splits in STEP_CASES:
        for rh in splits:
            cfg = arch_config(arch, 224)
            cfg.MODEL.ROPE_STAGES.NUM_HEADS = list(rh)
            cfg.DATA.TASK_KEYS_H5 = [t for t, _ in TASKS]
            cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in TASKS}
            model = build_model(cfg, num_classes={t: c for t, c in TASKS}).cuda()
            model.set_compute_dtype("bf16")
            model.train()
            g = torch.Generator().manual_seed(0)
            x = torch.rand(B, 3, 224, 224, generator=g).cuda()
            meta = (torch.rand(B, sum(model.meta_dims), generator=g) * 2 - 1).cuda() if model.meta_dims else None
            targets = {t: torch.randint(0, c, (B,), generator=g).cuda() for t, c in TASKS}

            def step():
                out = model(x, meta)
                multitask_cross_entropy(out, targets).backward()

            t = timed(step, a.steps, a.warmup)
            hd = [d // h for d, h in zip(cfg.MODEL.ROPE_STAGES.DIMS, rh)]
            key = f"{arch}[{rh[0]},{rh[1]}]"
            res["steps"][key] = {"batch": B, "head_dim": hd, "step_ms": round(t * 1e3, 2)}
            print(f"{key:14s} B={B} head_dim {hd}: {t * 1e3:8.2f} ms/step", flush=True)
            del model, x, meta
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["ops", "steps", "all"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--op-steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(), "ops": {}, "steps": {}}
    if a.part in ("ops", "all"):
        bench_ops(a, res)
    if a.part in ("steps", "all"):
        bench_steps(a, res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
