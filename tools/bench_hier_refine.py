#!/usr/bin/env python3
"""What the hierarchical refinement (MODEL.CLASSIFICATION.HIERARCHICAL_REFINEMENT) costs per train step: the device path
(linnaeus_amd.heads.HierarchicalRefinement: lnx_hier_refine_fwd / lnx_hier_refine_bwd, one launch per direction) against the torch
composition (linnaeus_amd.heads.refine_logits_top_down: per level a softmax, the membership GEMM through lnx_gemm_nt, a log, and
autograd's replay with the data-gradient GEMM, the unread weight-gradient GEMM and a padded transposed copy of the matrix), in ONE
process, the two legs alternated `--repeats` times, medians reported.

Sizes:
  heads     the project's four heads, 1000 / 300 / 80 / 20 classes (bench.py), batch 64 (lg @384)
  taxonomy  four levels of 10 000 / 3 000 / 600 / 100 classes, batch 256

Per leg: forward + backward on fp32 leaf logits, seeded; the backward is torch.autograd.backward on fixed upstream gradients (no loss
kernels in the window); a host clock between two device synchronisations around `iters` calls, after a warm-up of both legs at that
size.  Every child has a seeded parent; soft routing, temperature 1.  Before timing, the two legs' outputs and gradients are compared
on the same inputs.  Beside the times: the FLOP of the three products the composition runs per level pair (2 B C_parent C_child each)
and the bytes the device path has to move (per level and direction about four rows of B x C fp32), both computed from the shapes.

One JSON line at the end; --log appends it and the per-repeat lines to a file.  There is no CPU path."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

SIZES = {
    "heads": ((1000, 300, 80, 20), 64, 100),        # classes finest first, batch, timed calls per leg and repeat
    "taxonomy": ((10000, 3000, 600, 100), 256, 10),
}


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=list(SIZES), choices=list(SIZES))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hier_refine.py needs the MI355X: there is no CPU path")
    from linnaeus_amd.heads import HierarchicalRefinement, refine_logits_top_down

    lines = []

    def say(msg):
        print(msg, file=sys.stderr, flush=True)
        lines.append(msg)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup}
    for name in args.sizes:
        Cs, B, iters = SIZES[name]
        T = len(Cs)
        g = torch.Generator().manual_seed(20251020)
        keys = [f"taxa_L{10 * (i + 1)}" for i in range(T)]
        heads = nn.ModuleDict()
        for t in range(T):
            m = nn.Module()
            m.temperature = 1.0
            if t < T - 1:
                M = torch.zeros(Cs[t + 1], Cs[t])
                M[torch.randint(0, Cs[t + 1], (Cs[t],), generator=g), torch.arange(Cs[t])] = 1.0
                m.register_buffer(f"hmatrix_{keys[t + 1]}_{keys[t]}", M)
            heads[keys[t]] = m
        heads = heads.to(dev)
        refine = HierarchicalRefinement(heads, keys)
        leaves = {k: (torch.randn(B, c, generator=g) * 2).to(dev).requires_grad_(True) for k, c in zip(keys, Cs)}
        ups = [torch.randn(B, c, generator=g).to(dev) for c in Cs]

        def leg(device_path, n):
            for _ in range(n):
                for v in leaves.values():
                    v.grad = None
                out = refine(leaves) if device_path else refine_logits_top_down(leaves, heads, keys)
                torch.autograd.backward([out[k] for k in keys], ups)
            return out

        for device_path in (False, True):
            leg(device_path, args.warmup)
        ref = leg(False, 1)
        ref_g = {k: v.grad.clone() for k, v in leaves.items()}
        got = leg(True, 1)
        out_diff = max(float((got[k] - ref[k]).abs().max()) for k in keys)
        grad_diff = max(float((leaves[k].grad - ref_g[k]).abs().max() / ref_g[k].abs().max()) for k in keys)
        rows = {False: [], True: []}
        for r in range(args.repeats):
            for device_path in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg(device_path, iters)
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) / iters * 1e6
                rows[device_path].append(round(us, 1))
                say(f"[bench_hier_refine] {name} B={B} classes={list(Cs)} repeat {r} {'device' if device_path else 'torch composition'}: {us:.1f} us / forward + backward")
        gemm_flop = sum(3 * 2 * B * Cs[t + 1] * Cs[t] for t in range(T - 1))
        dev_bytes = 2 * 4 * 4 * B * sum(Cs)
        dev_us, comp_us = median(rows[True]), median(rows[False])
        result[name] = {"classes": list(Cs), "B": B, "iters": iters, "torch_composition_us": comp_us, "device_us": dev_us,
                        "all_torch_composition_us": rows[False], "all_device_us": rows[True], "torch_over_device": round(comp_us / dev_us, 2),
                        "composition_gemm_gflop_per_call": round(gemm_flop / 1e9, 2), "device_bytes_per_call_mb": round(dev_bytes / 1e6, 2),
                        "device_call_gb_per_s": round(dev_bytes / dev_us / 1e3, 1),
                        "max_abs_output_difference": out_diff, "max_relative_gradient_difference": grad_diff}
    line = json.dumps(result)
    print(line, flush=True)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines + [line]) + "\n")


if __name__ == "__main__":
    main()
