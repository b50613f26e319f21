#!/usr/bin/env python3
"""What taxonomy-aware label smoothing costs without the [C, C] matrix: TaxonomyAwareLabelSmoothingCE.from_tables (the kernels form
each soft row from linnaeus_amd.loss.TaxonomySmoothingTables, LNX_CE_FORM_TAXONOMY) against the matrix form on the matrix
`tables.dense()` gives, in ONE process, the two legs alternated `--repeats` times, medians reported.

Per class count C (default 10 000 / 3 000 / 600 / 100, batch 256): a seeded forest with C finest classes under three further levels
(each a quarter of the one below), alpha 0.1, beta 1, uniform roots; fp32 logits, hard targets with a fifth of the rows null, a
class weight, null-mask probability 0.5, one task.

  build_ms    host time of build_taxonomy_smoothing_tables (what replaces the reference's build_distance_matrix +
              build_taxonomy_smoothing_matrix at start-up)
  bytes       anc + val against 4 C^2 for the matrix (the reference holds a second [C, C] tensor for the distances while it builds)
  dense_ms    tables.dense(): the whole matrix from the tables on the device (one launch), for whoever still wants it
  kernels_us  lnx_hier_loss_fwd + lnx_hier_loss_bwd (three launches) enqueued back to back, device events around `--iters` pairs
  call_us     weighted_hierarchical_loss(fused=True) forward + backward on leaf logits, host clock between two synchronisations
              (the host side of the call: three launches, one torch.rand and the Python around them)

The two forms give the same bits (checked here at every size).  `--table-only` sizes (default 50 000, whose matrix would be 10 GB)
report the table leg alone.  Every line goes to stdout and to `--log`; one JSON line at the end.  There is no CPU path."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from types import SimpleNamespace as NS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

CFG = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=False), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=True, VAL=False))))
TASK = "taxa_L10"


def median(v):
    return sorted(v)[len(v) // 2]


def forest(Cn, rng):
    ncls = [Cn] + [max(2, -(-Cn // 4 ** k)) for k in (1, 2, 3)]
    parents = [rng.integers(0, ncls[lv + 1], ncls[lv]) for lv in range(3)]
    for p in parents:
        p[rng.random(len(p)) < 0.05] = -1  # some parentless classes at every level
    return ncls, parents


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, nargs="+", default=[10000, 3000, 600, 100])
    ap.add_argument("--table-only", type=int, nargs="*", default=[50000])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "taxonomy_loss_bench.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_taxonomy_loss.py needs the MI355X: there is no CPU path")
    from linnaeus_amd import _lib as L
    from linnaeus_amd.loss import GradientWeighting, TaxonomyAwareLabelSmoothingCE, build_taxonomy_smoothing_tables, weighted_hierarchical_loss

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    log = open(args.log, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    B = args.batch
    sched = NS(get_null_mask_prob=lambda step: 0.5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    result = {"workload": f"one task, batch {B}, fp32 logits, depth-3 tables, class weight, null-mask probability 0.5; {args.warmup} warm-up + {args.iters} "
                          f"timed iterations per leg, {args.repeats} alternated repeats, median"}
    for Cn in list(args.classes) + list(args.table_only):
        legs = ("table",) if Cn in args.table_only and Cn not in args.classes else ("matrix", "table")
        rng = np.random.default_rng(Cn)
        ncls, parents = forest(Cn, rng)
        t0 = time.perf_counter()
        tables = build_taxonomy_smoothing_tables(parents, ncls, 0, 0.1, 1.0, True)
        build_ms = (time.perf_counter() - t0) * 1e3
        g = torch.Generator(device=dev).manual_seed(Cn)
        w = 0.5 + torch.rand(Cn, device=dev, generator=g)
        x = torch.randn(B, Cn, device=dev, generator=g) * 2
        y = torch.randint(0, Cn, (B,), device=dev, generator=g)
        y[torch.rand(B, device=dev, generator=g) < 0.2] = 0
        crit = {"table": TaxonomyAwareLabelSmoothingCE.from_tables(tables, weight=w, apply_class_weights=True).to(dev)}
        dense_ms = None
        if "matrix" in legs:
            tables.dense()  # (warm-up: code object, upload)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m = tables.dense()
            torch.cuda.synchronize()
            dense_ms = (time.perf_counter() - t0) * 1e3
            crit["matrix"] = TaxonomyAwareLabelSmoothingCE(m, weight=w, apply_class_weights=True).to(dev)
            del m
        for c in crit.values():
            c.validate_targets = False
        cw = {i: 0.5 + (i % 7) / 7.0 for i in range(0, Cn, 2)}
        gw = {k: GradientWeighting([TASK], CFG, "static", init_weights={TASK: 0.7}, class_weights={TASK: cw}) for k in legs}
        leaf = x.clone().requires_grad_(True)
        outputs, targets = {TASK: leaf}, {TASK: y}
        criteria = {k: {TASK: crit[k]} for k in legs}  # (the fused loss is built once per criteria dict and kept on the task weighting)

        def call(kind, n):
            for _ in range(n):
                leaf.grad = None
                weighted_hierarchical_loss(outputs, targets, criteria[kind], gw[kind], sched, 0, config=CFG, sync_components=False, fused=True)[0].backward()

        # the raw launches: the arguments FusedHierarchicalLoss would fill, kept alive here
        vec = torch.ones(Cn, device=dev)
        for i, v in cw.items():
            vec[i] = v
        draws, weights, go = torch.rand(1, B, device=dev, generator=g), torch.full((1,), 0.7, device=dev), torch.ones(1, device=dev)
        raw = {}
        for kind in legs:
            ws, out = torch.empty(L.HL_WS_ROWS, B, device=dev), torch.zeros(L.HL_OUT_FLOATS, device=dev)
            counts, d = torch.zeros(L.HL_COUNTS, dtype=torch.int64, device=dev), torch.empty(B, Cn, device=dev)
            a = L.HierLossArgs()
            a.dtype, a.B, a.n_tasks, a.prob, a.mask_mul = L.F32, B, 1, 0.5, 0
            a.draws, a.weights, a.ws, a.out, a.counts = draws.data_ptr(), weights.data_ptr(), ws.data_ptr(), out.data_ptr(), counts.data_ptr()
            k = a.task[0]
            k.logits, k.ld, k.C, k.target, k.ignore_index = x.data_ptr(), x.stride(0), Cn, y.data_ptr(), -1
            k.crit_weight, k.class_weight, k.n_cw, k.p_cw, k.p_w = w.data_ptr(), vec.data_ptr(), Cn, 2, 3
            k.dlogits, k.ldd = d.data_ptr(), d.stride(0)
            soft, form, tax = crit[kind]._row_source(dev)
            k.form, k.soft = form, (soft.data_ptr() if soft is not None else None)
            if tax is not None:
                k.tax_anc, k.tax_val, k.tax_depth = tax[0].data_ptr(), tax[1].data_ptr(), tax[2]
            raw[kind] = (a, ws, out, counts, d)

        def kernels(kind, n):
            a = raw[kind][0]
            for _ in range(n):
                L.check(L.lib().lnx_hier_loss_fwd(C.byref(a), stream), "lnx_hier_loss_fwd")
                L.check(L.lib().lnx_hier_loss_bwd(C.byref(a), C.c_void_p(go.data_ptr()), stream), "lnx_hier_loss_bwd")

        for kind in legs:
            call(kind, args.warmup)
            kernels(kind, args.warmup)
        torch.cuda.synchronize()
        same = None
        if "matrix" in legs:  # faster and different is not faster: the two forms give the same bits
            same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(raw["matrix"][1:], raw["table"][1:]) if p.dtype == torch.float32)
            grads = {}
            for kind in legs:
                torch.manual_seed(1)
                call(kind, 1)
                grads[kind] = leaf.grad.clone()
            same = same and torch.equal(grads["matrix"].view(torch.int32), grads["table"].view(torch.int32))
        rows = {(kind, what): [] for kind in legs for what in ("kernels_us", "call_us")}
        for r in range(args.repeats):
            for kind in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                kernels(kind, args.iters)
                e1.record()
                torch.cuda.synchronize()
                rows[(kind, "kernels_us")].append(round(e0.elapsed_time(e1) * 1e3 / args.iters, 2))
                t0 = time.perf_counter()
                call(kind, args.iters)
                torch.cuda.synchronize()
                rows[(kind, "call_us")].append(round((time.perf_counter() - t0) / args.iters * 1e6, 2))
        rec = {"build_ms": round(build_ms, 3), "table_bytes": tables.nbytes, "matrix_bytes": tables.matrix_bytes, "dense_ms": dense_ms and round(dense_ms, 3),
               "same_bits": same}
        for (kind, what), v in rows.items():
            rec[f"{kind}_{what}"] = median(v)
            rec[f"all_{kind}_{what}"] = v
        result[f"C{Cn}"] = rec
        line = f"[bench_taxonomy_loss] C={Cn} B={B}: tables built in {build_ms:.2f} ms, {tables.nbytes} bytes against {tables.matrix_bytes} for the matrix"
        if "matrix" in legs:
            ratio = rec["table_kernels_us"] / rec["matrix_kernels_us"]
            line += (f"; dense() {dense_ms:.2f} ms; kernels fwd + bwd {rec['table_kernels_us']:.1f} us with tables, {rec['matrix_kernels_us']:.1f} us with the matrix "
                     f"(tables / matrix = {ratio:.2f}); call {rec['table_call_us']:.1f} us with tables, {rec['matrix_call_us']:.1f} us with the matrix; same bits: {same}")
        else:
            line += f"; kernels fwd + bwd {rec['table_kernels_us']:.1f} us, call {rec['table_call_us']:.1f} us with tables (no matrix leg: it would not fit a sensible budget)"
        say(line)
        del crit, raw, gw, leaf, criteria, outputs
        torch.cuda.empty_cache()
    say(json.dumps(result))
    log.close()


if __name__ == "__main__":
    main()
