#!/usr/bin/env python3
"""What validating K metadata variants of the same images costs on mFormerV1_sm (eval batch 512, bf16, 224 px, the three shipped
metadata components), K = 2 (`val` + `val_mask_meta`) and K = 4 (+ `val_mask_TEMPORAL`, `val_mask_SPATIAL_ELEVATION`).

The `throughput_test` protocol of bench.py --eval (eval mode, no_grad, resident uniform-random inputs, warm-up calls, then timed calls
between two device synchronisations), `--repeats` alternated repeats, median.  Two legs, each a process of its own:

  --leg a   K plain `model(x, m_k)` calls: the public forward only, so it runs on an OLDER build of the library
            (LNX_LIB_PATH=<the parent commit's liblnx_hip.so> LNX_LIB_OLDER=1).  It also records, per forward, what the plan's
            block-level profile (lnx_plan_profile_begin_spans / lnx_plan_profile_end_ex) knows of the trunk: the ConvNeXt-block spans
            (class 9) and the RoPE-block spans (class 8).  The stem and the downsample products have no span class of their own, so two
            trunk figures are given: `trunk_conv_spans_ms` (the conv blocks alone: a LOWER bound of the trunk) and
            `trunk_outside_rope_ms` = forward - RoPE-block spans (an UPPER bound: it also holds the weight refresh, norm_1, downsample 2,
            the tail and the heads, none of which a tail saves).
  --leg b   one `forward_meta_variants(x, metas)`; first checks that every variant is torch.equal to its plain forward.  With
            --parent <json of leg a> it evaluates  b <= a - 0.5 (K - 1) trunk  for both K and BOTH trunk figures.

One JSON line at the end of each leg."""
import argparse
import ctypes as C
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
COMBOS = [(), None, ["TEMPORAL"], ["SPATIAL", "ELEVATION"]]
KS = (2, 4)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", required=True, choices=["a", "b"])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile-steps", type=int, default=10)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"])
    ap.add_argument("--parent", default=None, help="leg b: the JSON line leg a printed on the parent build, for the acceptance check")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_meta_variants.py needs the MI355X: there is no CPU path")
    from linnaeus_amd import _lib as L
    from linnaeus_amd import arch_config, build_model
    from linnaeus_amd.collate import mask_meta_components

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(42)
    keys = [t for t, _ in TASKS]
    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = keys
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t in keys}
    for comp in ("TEMPORAL", "SPATIAL", "ELEVATION"):  # (the default config ships ELEVATION switched off)
        cfg.DATA.META.COMPONENTS[comp].ENABLED = True
    model = build_model(cfg, num_classes=dict(TASKS)).to(dev).eval()
    model.set_compute_dtype(args.dtype)
    names = list(model.meta_components)
    if names != ["TEMPORAL", "SPATIAL", "ELEVATION"]:
        sys.exit(f"expected the three shipped metadata components, the sm config has {names}")
    bounds = {n: (i["offset"], i["offset"] + i["dim"]) for n, i in model.meta_components.items()}
    g = torch.Generator(device=dev).manual_seed(42)
    B = args.batch
    x = torch.rand(B, 3, 224, 224, device=dev, generator=g)
    aux = torch.rand(B, sum(model.meta_dims), device=dev, generator=g)
    # (built from the masking call every build has: leg a runs on builds without collate.meta_variants)
    metas = [aux if c == () else mask_meta_components(aux, bounds, None if c is None else list(c)) for c in COMBOS]
    lib = L.lib()

    def run(K, n):
        for _ in range(n):
            if args.leg == "a":
                for k in range(K):
                    model(x, metas[k])
            else:
                model.forward_meta_variants(x, metas[:K])

    def timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    res = {"leg": args.leg, "lnx_version": lib.lnx_version(), "library": os.path.join(os.path.basename(os.path.dirname(L.LIB_PATH)), os.path.basename(L.LIB_PATH)),
           "workload": f"mFormerV1_sm 3x224x224 eval forward, batch {B}, {args.dtype}, no_grad, components {names}; {args.warmup} warm-up + "
                       f"{args.iters} timed calls, {args.repeats} alternated repeats, median"}
    rows = {K: [] for K in KS}
    fwd_rows = []
    with torch.no_grad():
        if args.leg == "b":
            outs = model.forward_meta_variants(x, metas)
            res["bit_equal_to_plain_forwards"] = all(torch.equal(o[t], p[t]) for o, m in zip(outs, metas) for p in [model(x, m)] for t in keys)
            if not res["bit_equal_to_plain_forwards"]:
                sys.exit("forward_meta_variants differs from the plain forwards")
        for K in KS:
            run(K, args.warmup)
        for r in range(args.repeats):
            for K in KS:
                ms = timed(lambda n: run(K, n), args.iters)
                rows[K].append(round(ms, 4))
                print(f"[bench_meta_variants] repeat {r} leg {args.leg} K={K}: {ms:.4f} ms / batch", file=sys.stderr, flush=True)
            fwd_rows.append(round(timed(lambda n: [model(x, metas[0]) for _ in range(n)], args.iters), 4))
        for K in KS:
            res[f"K{K}_ms"] = median(rows[K])
        res["forward_ms"] = median(fwd_rows)
        res["all_repeats_ms"] = {"forward": fwd_rows, **{f"K{K}": rows[K] for K in KS}}
        # the block-level spans of the plain forward (untimed extra calls: the events sit on the launch stream)
        model(x, metas[0])
        st = model._active
        NC = 10
        L.check(lib.lnx_plan_profile_begin_spans(st["handle"]), "lnx_plan_profile_begin_spans")
        for _ in range(args.profile_steps):
            model(x, metas[0])
        ms, work, byts, cnt = (C.c_double * NC)(), (C.c_double * NC)(), (C.c_double * NC)(), (C.c_int * NC)()
        L.check(lib.lnx_plan_profile_end_ex(st["handle"], ms, work, byts, cnt), "lnx_plan_profile_end_ex")
        n = args.profile_steps
        res["spans_per_forward"] = {"conv_block_ms": round(ms[9] / n, 4), "conv_blocks": cnt[9] // n, "rope_block_ms": round(ms[8] / n, 4), "rope_blocks": cnt[8] // n}
        res["trunk_conv_spans_ms"] = round(ms[9] / n, 4)
        res["trunk_outside_rope_ms"] = round(res["forward_ms"] - ms[8] / n, 4)
        if args.leg == "b":
            # the same spans over one forward_meta_variants(K = 4): the conv blocks once, the RoPE blocks four times
            L.check(lib.lnx_plan_profile_begin_spans(st["handle"]), "lnx_plan_profile_begin_spans")
            for _ in range(n):
                model.forward_meta_variants(x, metas)
            L.check(lib.lnx_plan_profile_end_ex(st["handle"], ms, work, byts, cnt), "lnx_plan_profile_end_ex")
            res["spans_per_variants_call_K4"] = {"conv_block_ms": round(ms[9] / n, 4), "conv_blocks": cnt[9] // n, "rope_block_ms": round(ms[8] / n, 4),
                                                 "rope_blocks": cnt[8] // n}
    if args.leg == "b" and args.parent:
        with open(args.parent) as fh:
            par = json.loads([ln for ln in fh.read().splitlines() if ln.startswith("{")][-1])
        acc = {}
        for K in KS:
            a, b = par[f"K{K}_ms"], res[f"K{K}_ms"]
            for which in ("trunk_conv_spans_ms", "trunk_outside_rope_ms"):
                bound = a - 0.5 * (K - 1) * par[which]
                acc[f"K{K}_vs_{which}"] = {"a_ms": a, "b_ms": b, "trunk_ms": par[which], "bound_ms": round(bound, 4), "saved_ms": round(a - b, 4),
                                           "saved_trunks": round((a - b) / ((K - 1) * par[which]), 3), "met": bool(b <= bound)}
        res["acceptance"] = acc
        res["parent"] = {k: par[k] for k in ("lnx_version", "library", "forward_ms", "K2_ms", "K4_ms", "spans_per_forward", "trunk_conv_spans_ms", "trunk_outside_rope_ms")}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
