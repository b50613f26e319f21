"""One GradNorm update (GradientWeighting.update_gradnorm_weights_reforward) on mFormerV1_sm against the reference's recipe run on
the same model, with a training step for context.

    python tools/bench_gradnorm.py [--batch 256] [--steps 10] [--warmup 3] [--dtype bf16] [--recompute 0]

  ours       one forward of the native plan, T lnx_plan_backward_into into a scratch arena, lnx_gradnorm_sumsq per task and
             lnx_gradnorm_update; no host sync (sync=False)
  reference  what gradient_weighting.py:367-880 does per task, written out here: a forward, the task's masked mean loss,
             torch.autograd.grad over the backbone parameters, torch.cat of the gradients and its norm (+ one .item() per task,
             as the reference's loss bookkeeping does); without its gc.collect() / empty_cache() calls
  step       forward + multi-task loss + backward (autograd grad mode), for scale

Four Linear heads (1000 / 300 / 80 / 20 classes), T = 4, 224 px.  Times are device-synchronised wall clock per call after
warm-up.  Last line: one JSON object with every number.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linnaeus_amd import arch_config, build_model  # noqa: E402
from linnaeus_amd.config import ConfigNode  # noqa: E402
from linnaeus_amd.loss import DEFAULT_EXCLUDE_CONFIG, GradientWeighting, TaxonomyAwareLabelSmoothingCE, multitask_cross_entropy  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--recompute", type=int, default=0, help="TRAIN.GRADIENT_CHECKPOINTING.ENABLED_GRADNORM_STEPS")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gradnorm needs the GPU"
    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = [t for t, _ in TASKS]
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in TASKS}
    cfg.LOSS = ConfigNode({"GRAD_WEIGHTING": {"TASK": {"TYPE": "gradnorm", "ALPHA": 1.5, "ZERO_AUX_INFO": True, "GRADNORM_ACCUM_STEPS": 1,
                                                       "EXCLUDE_CONFIG": DEFAULT_EXCLUDE_CONFIG}}})
    cfg.TRAIN.GRADIENT_CHECKPOINTING.ENABLED_GRADNORM_STEPS = bool(a.recompute)
    model = build_model(cfg, num_classes={t: c for t, c in TASKS}).cuda()
    model.set_compute_dtype(a.dtype)
    model.train()
    B = a.batch
    g = torch.Generator().manual_seed(0)
    x = torch.rand(B, 3, 224, 224, generator=g).cuda()
    meta = (torch.rand(B, sum(model.meta_dims), generator=g) * 2 - 1).cuda() if model.meta_dims else None
    targets = {t: torch.randint(0, c, (B,), generator=g).cuda() for t, c in TASKS}
    crit = {t: TaxonomyAwareLabelSmoothingCE(torch.eye(c) * 0.9 + 0.1 / c).cuda() for t, c in TASKS}
    for c in crit.values():
        c.validate_targets = False
    gw = GradientWeighting([t for t, _ in TASKS], cfg, "gradnorm")
    gw.set_model(model)

    ours = timed(lambda: gw.update_gradnorm_weights_reforward((x, targets, meta), crit, sync=False, keep_step_grads=True), a.steps, a.warmup)

    bb = gw.backbone_params
    zmeta = torch.zeros_like(meta) if meta is not None else None

    def reference():
        for t, _ in TASKS:
            out = model(x, zmeta, force_checkpointing=bool(a.recompute))
            valid = targets[t] != 0
            n = int(valid.sum().item())
            loss = crit[t](out[t], targets[t])[valid].sum() / max(n, 1)
            grads = torch.autograd.grad(loss, bb, allow_unused=True)
            flat = torch.cat([(gg if gg is not None else torch.zeros_like(p)).flatten() for gg, p in zip(grads, bb)]).float()
            flat.norm()

    ref = timed(reference, a.steps, a.warmup)

    def step():
        out = model(x, meta)
        loss = multitask_cross_entropy(out, targets)
        loss.backward()

    st = timed(step, a.steps, a.warmup)
    res = {"arch": "mFormerV1_sm", "batch": B, "tasks": len(TASKS), "dtype": a.dtype, "recompute": bool(a.recompute), "steps": a.steps,
           "gradnorm_update_ms": round(ours, 3), "reference_recipe_ms": round(ref, 3), "speedup": round(ref / ours, 3), "train_step_ms": round(st, 3)}
    print(f"GradNorm update (ours)          {ours:9.2f} ms")
    print(f"reference recipe (T fwd+grad)   {ref:9.2f} ms   ({ref / ours:.2f}x)")
    print(f"training step, for scale        {st:9.2f} ms")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
