#!/usr/bin/env python3
"""What the validation loop's metric bookkeeping costs around the eval forward of mFormerV1_sm (batch 512, bf16, 224 px).

The `throughput_test` protocol of bench.py --eval (eval mode, no_grad, resident uniform-random inputs, warm-up calls, then timed calls
between two device synchronisations), three legs in ONE process, alternated `--repeats` times so that drift hits all of them alike:

  a  forward only
  b  forward + the torch operations and host reads of the reference's MetricsTracker._update_phase_batch, restated here from its
     description: per task an argmax for the chain figure, one for the partial chain figure and one for acc1, topk(3) for acc3, the
     stacks / masks of the two chain figures, and one .item() per figure (1 chain, 2 partial chain, 2 per task, 6 per null-tracked task
     with its per-sample losses).  Index targets ([B]), which spares this leg the argmax over one-hot targets the reference also pays;
     no logging, no subset wrappers: the lightest form of that bookkeeping.
  c  forward + DeviceMetrics.update (one lnx_metrics_update launch, no host read), one compute() after the last call, inside the
     timed window.

Also: `update` alone, enqueued back to back between two events (an upper bound of the kernel's time: launch-rate bound when the
kernel is shorter than a launch).  --kernel-only runs just that loop, for a kernel trace of its own.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
NULL_TASKS = ("taxa_L10", "taxa_L20")


def torch_bookkeeping(acc, keys, outputs, targets, losses):
    """Leg b: the reference's per-batch update as torch ops + .item() reads, accumulating into the host dict `acc`."""
    B = outputs[keys[0]].shape[0]
    # chain accuracy: argmax per task, stack, all, one read
    eq = torch.stack([outputs[t].argmax(dim=1) == targets[t] for t in keys], dim=1)
    acc["chain_correct"] += eq.all(dim=1).sum().item() / B * B
    acc["chain_total"] += B
    # partial chain accuracy: argmax per task again, highest non-null rank, two reads
    eq = torch.stack([outputs[t].argmax(dim=1) == targets[t] for t in keys], dim=1)
    gts = torch.stack([targets[t] for t in keys], dim=1)
    ranks = torch.arange(len(keys), device=gts.device).expand(B, -1)
    highest = ranks.masked_fill(~(gts != 0), -1).max(dim=1)[0]
    has = highest >= 0
    ok = torch.logical_or(~(ranks <= highest.unsqueeze(1)), eq).all(dim=1) & has
    n_ok, n_has = ok.sum().item(), has.sum().item()
    acc["partial_correct"] += (n_ok / n_has if n_has else 1.0) * B
    acc["partial_total"] += B
    # per task acc1 / acc3: argmax a third time, topk(3), two reads
    for t in keys:
        out, gt = outputs[t], targets[t]
        acc[f"c1_{t}"] += (out.argmax(dim=1) == gt).sum().item()
        acc[f"c3_{t}"] += (out.topk(3, dim=1)[1] == gt.unsqueeze(1)).any(dim=1).sum().item()
        acc[f"n_{t}"] += B
    # null / non-null split: six reads per tracked task
    for t in NULL_TASKS:
        gt, ls = targets[t], losses[t]
        null = gt == 0
        non = ~null
        n_null, n_non = null.sum().item(), non.sum().item()
        if n_null:
            acc[f"null_c1_{t}"] += ((outputs[t].argmax(dim=1) == gt) & null).sum().item()
            acc[f"null_loss_{t}"] += ls[null].sum().item()
        if n_non:
            acc[f"non_c1_{t}"] += ((outputs[t].argmax(dim=1) == gt) & non).sum().item()
            acc[f"non_loss_{t}"] += ls[non].sum().item()
        acc[f"null_n_{t}"] += n_null
        acc[f"non_n_{t}"] += n_non


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--kernel-only", action="store_true", help="only the back-to-back update loop (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_metrics.py needs the MI355X: there is no CPU path")
    from collections import defaultdict

    from linnaeus_amd import arch_config, build_model
    from linnaeus_amd.metrics import DeviceMetrics

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(42)
    keys = [t for t, _ in TASKS]
    g = torch.Generator(device=dev).manual_seed(42)
    B = args.batch
    targets = {t: torch.randint(0, c, (B,), device=dev, generator=g) for t, c in TASKS}
    for t in keys:
        targets[t][torch.rand(B, device=dev, generator=g) < 0.2] = 0
    losses = {t: torch.rand(B, device=dev, generator=g) * 3 for t in keys}
    dm = DeviceMetrics(keys, dict(TASKS), null_tracking_tasks=NULL_TASKS)

    def update_loop(outputs, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        dm.reset()
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            dm.update(outputs, targets, per_sample_losses=losses)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3  # us per call

    if args.kernel_only:
        dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
        outputs = {t: torch.randn(B, c, device=dev, generator=g).to(dt) for t, c in TASKS}
        update_loop(outputs, 20)
        print(json.dumps({"update_enqueued_us": round(update_loop(outputs, 200), 3), "batch": B, "dtype": args.dtype}), flush=True)
        return

    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = keys
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t in keys}
    model = build_model(cfg, num_classes=dict(TASKS)).to(dev).eval()
    model.set_compute_dtype(args.dtype)
    meta_width = sum(model.meta_dims)
    x = torch.rand(B, 3, 224, 224, device=dev, generator=g)
    meta = torch.rand(B, meta_width, device=dev, generator=g) if meta_width else None
    acc = defaultdict(float)

    def leg(name, n):
        if name == "c":
            dm.reset()
        for _ in range(n):
            out = model(x, meta)
            if name == "b":
                torch_bookkeeping(acc, keys, out, targets, losses)
            elif name == "c":
                dm.update(out, targets, per_sample_losses=losses)
        return dm.compute() if name == "c" else None

    rows = {k: [] for k in "abc"}
    with torch.no_grad():
        for name in "abc":
            leg(name, args.warmup)
        torch.cuda.synchronize()
        for r in range(args.repeats):
            for name in "abc":
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = leg(name, args.iters)
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / args.iters * 1e3
                rows[name].append(round(ms, 4))
                print(f"[bench_metrics] repeat {r} leg {name}: {ms:.4f} ms / batch, {B / ms * 1e3:.0f} img/s", file=sys.stderr, flush=True)
        out = model(x, meta)
        # the two bookkeepings counted the same things (same outputs every call)
        acc.clear()
        torch_bookkeeping(acc, keys, out, targets, losses)
        dm.reset()
        dm.update(out, targets, per_sample_losses=losses)
        res = dm.compute()
        agree = all(acc[f"c1_{t}"] == res["counts"]["tasks"][t]["correct1"] for t in keys) and round(acc["chain_correct"]) == res["counts"]["chain_correct"]
        upd_us = update_loop(out, 200)
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    print(json.dumps({
        "workload": f"mFormerV1_sm 3x224x224 eval forward, batch {B}, {args.dtype}, no_grad; {args.warmup} warm-up + {args.iters} timed calls per leg, "
                    f"{args.repeats} alternated repeats, median",
        "a_forward_ms": med["a"], "b_forward_plus_torch_bookkeeping_ms": med["b"], "c_forward_plus_device_metrics_ms": med["c"],
        "b_minus_a_ms": round(med["b"] - med["a"], 4), "c_minus_a_ms": round(med["c"] - med["a"], 4),
        "update_enqueued_back_to_back_us": round(upd_us, 3), "all_repeats_ms": rows, "torch_and_device_counts_agree": bool(agree),
        "host_reads_per_batch_leg_b": 3 + 2 * len(keys) + 6 * len(NULL_TASKS)}), flush=True)


if __name__ == "__main__":
    main()
