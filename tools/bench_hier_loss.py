#!/usr/bin/env python3
"""What the hierarchical loss costs in a train step of mFormerV1_sm: the composed path of linnaeus_amd.loss.weighted_hierarchical_loss
(one lnx_softce launch per task, then torch operations on [B] vectors, replayed by autograd) against fused=True (lnx_hier_loss_fwd /
lnx_hier_loss_bwd: two launches forward, one backward), in ONE process, the two legs alternated `--repeats` times, medians reported.

Shapes: the four heads of mFormerV1_sm (1000 / 300 / 80 / 20 classes), batch 256 and 128, fp32 logits as column slices of wider
rows (the pitch the model's plan hands out is padded), hard targets with a fifth of the rows null, class weights, scheduled null
masking with inclusion probability 0.5 (the path with the most work: one torch.rand per task in both legs), sync_components=False.

  loss   forward + backward of the loss alone on leaf logits, host clock between two device synchronisations
  step   (--step) model forward + loss + backward of mFormerV1_sm at 224 px in bf16; the difference of the two legs is the gap the
         loss leaves between the last forward kernel and the first backward kernel

--criteria picks the per-task criterion of both legs (the composed leg runs the same classes in the same process): `taxonomy`
(TaxonomyAwareLabelSmoothingCE, the default), `ce` (CrossEntropyLoss, the reference's default configuration), `ls`
(LabelSmoothingCrossEntropy, smoothing 0.1) or `st` (SoftTargetCrossEntropy on [B, C] mixup rows, 0.6 / 0.4 of two samples' labels);
the last three carry a class weight of their own.

One JSON line at the end.  There is no CPU path."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace as NS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
CFG = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=False), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=True, VAL=False))))


def median(v):
    return sorted(v)[len(v) // 2]


def mixup_rows(targets, B, dev, g):
    """[B, C] rows: 0.6 of each sample's label and 0.4 of another sample's"""
    perm = torch.randperm(B, device=dev, generator=g)
    out = {}
    for t, c in TASKS:
        one = torch.nn.functional.one_hot(targets[t], c).float()
        out[t] = 0.6 * one + 0.4 * one[perm]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 128])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="also time the whole train step of mFormerV1_sm around the two paths")
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--criteria", choices=("taxonomy", "ce", "ls", "st"), default="taxonomy", help="the per-task criterion of both legs")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hier_loss.py needs the MI355X: there is no CPU path")
    from linnaeus_amd.loss import (CrossEntropyLoss, GradientWeighting, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy, TaxonomyAwareLabelSmoothingCE,
                                   weighted_hierarchical_loss)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(42)
    keys = [t for t, _ in TASKS]
    g = torch.Generator(device=dev).manual_seed(42)
    crit, cw = {}, {}
    for t, c in TASKS:
        m = 0.9 * torch.eye(c, device=dev) + 0.1 * torch.softmax(torch.randn(c, c, device=dev, generator=g), 1)
        w = 0.5 + torch.rand(c, device=dev, generator=g)
        if args.criteria == "taxonomy":
            crit[t] = TaxonomyAwareLabelSmoothingCE(m / m.sum(1, keepdim=True)).to(dev)
        elif args.criteria == "ce":
            crit[t] = CrossEntropyLoss(w, True)
        elif args.criteria == "ls":
            crit[t] = LabelSmoothingCrossEntropy(w, 0.1, True)
        else:
            crit[t] = SoftTargetCrossEntropy(w, True)
        crit[t].validate_targets = False  # no host read in the step
        cw[t] = {i: 0.5 + (i % 7) / 7.0 for i in range(0, c, 2)}
    gw = GradientWeighting(keys, CFG, "static", init_weights={t: 1.0 / (i + 1) for i, t in enumerate(keys)}, class_weights=cw)
    sched = NS(get_null_mask_prob=lambda step: 0.5)
    result = {"criteria": args.criteria,
              "workload": f"weighted_hierarchical_loss, heads {[c for _, c in TASKS]}, fp32 padded logits, class weights, null-mask probability 0.5; "
                          f"{args.warmup} warm-up + {args.iters} timed calls per leg, {args.repeats} alternated repeats, median"}

    def loss_of(outputs, targets, fused):
        return weighted_hierarchical_loss(outputs, targets, crit, gw, sched, 0, config=CFG, sync_components=False, fused=fused)[0]

    for B in args.batches:
        targets = {t: torch.randint(0, c, (B,), device=dev, generator=g) for t, c in TASKS}
        for t in keys:
            targets[t][torch.rand(B, device=dev, generator=g) < 0.2] = 0
        if args.criteria == "st":
            targets = mixup_rows(targets, B, dev, g)
        wide = {t: torch.randn(B, (c + 15) // 16 * 16 + 16, device=dev, generator=g) * 2 for t, c in TASKS}
        leaves = {t: wide[t][:, :c].detach().requires_grad_(True) for t, c in TASKS}

        def leg(fused, n):
            for _ in range(n):
                for v in leaves.values():
                    v.grad = None
                loss_of(leaves, targets, fused).backward()

        for fused in (False, True):
            leg(fused, args.warmup)
        # the two legs computed the same thing
        torch.manual_seed(1)
        leg(False, 1)
        ref = {t: v.grad.clone() for t, v in leaves.items()}
        torch.manual_seed(1)
        leg(True, 1)
        worst = max(float((leaves[t].grad - ref[t]).abs().max() / ref[t].abs().max()) for t in keys)
        rows = {False: [], True: []}
        for r in range(args.repeats):
            for fused in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg(fused, args.iters)
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) / args.iters * 1e6
                rows[fused].append(round(us, 2))
                print(f"[bench_hier_loss] B={B} repeat {r} {'fused' if fused else 'composed'}: {us:.1f} us / forward + backward", file=sys.stderr, flush=True)
        result[f"loss_B{B}"] = {"composed_us": median(rows[False]), "fused_us": median(rows[True]), "all_composed_us": rows[False], "all_fused_us": rows[True],
                                "worst_relative_gradient_difference": worst}

    if args.step:
        from linnaeus_amd import arch_config, build_model

        cfg = arch_config("sm", 224)
        cfg.DATA.TASK_KEYS_H5 = keys
        cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t in keys}
        model = build_model(cfg, num_classes=dict(TASKS)).to(dev).train()
        model.set_compute_dtype("bf16")
        meta_width = sum(model.meta_dims)
        for B in args.batches:
            x = torch.rand(B, 3, 224, 224, device=dev, generator=g)
            meta = torch.rand(B, meta_width, device=dev, generator=g) if meta_width else None
            targets = {t: torch.randint(0, c, (B,), device=dev, generator=g) for t, c in TASKS}
            if args.criteria == "st":
                targets = mixup_rows(targets, B, dev, g)

            def step(fused, n):
                for _ in range(n):
                    model.zero_grad(set_to_none=True)
                    loss_of(model(x, meta), targets, fused).backward()

            for fused in (False, True):
                step(fused, 3)
            rows = {False: [], True: []}
            for r in range(args.repeats):
                for fused in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    step(fused, args.step_iters)
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) / args.step_iters * 1e3
                    rows[fused].append(round(ms, 3))
                    print(f"[bench_hier_loss] step B={B} repeat {r} {'fused' if fused else 'composed'}: {ms:.3f} ms", file=sys.stderr, flush=True)
            result[f"step_B{B}"] = {"composed_ms": median(rows[False]), "fused_ms": median(rows[True]),
                                    "composed_minus_fused_ms": round(median(rows[False]) - median(rows[True]), 3), "all_composed_ms": rows[False],
                                    "all_fused_ms": rows[True]}
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
