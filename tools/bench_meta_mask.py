#!/usr/bin/env python3
"""What the scheduled metadata masking of the collate step costs on a device batch (B = 256, D = 15: TEMPORAL 0:2, SPATIAL 2:5,
ELEVATION 5:15; p_full 0.3, partial masking on with p_partial 0.7 and the six-combination weighted whitelist of the example
experiment), with the per-component statistics that follow it.

Three legs in ONE process, alternated `--repeats` times so that drift hits all of them alike; every leg starts from fresh clones of
the same batch, runs `--iters` batches between two device synchronisations and is reported per batch (host wall clock: the loop of
leg a is host-bound, so device events would miss most of it):

  a   the reference's bookkeeping as torch ops on the device batch, restated literally (h5data/h5dataloader.py:709-940, 1740-1801):
      two torch.rand(B), the indexed full mask, a Python loop over the rows that reads two device scalars per row, a cloned and
      re-assigned row per partial mask, then one .item() per component for the statistics
  b   the same result from batched torch ops without a per-row loop (searchsorted pick, one where per tensor), statistics kept on
      the device
  c   GPUMetaMasking.__call__ + stats(): one torch.rand(3, B), one lnx_meta_mask launch each, nothing read back

Also: leg c's two launches enqueued back to back between two events (an upper bound of the kernels' time: launch-rate bound when a
kernel is shorter than a launch).  One JSON line at the end."""
import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

BOUNDS = {"TEMPORAL": (0, 2), "SPATIAL": (2, 5), "ELEVATION": (5, 15)}
WHITELIST = [["TEMPORAL"], ["SPATIAL"], ["ELEVATION"], ["TEMPORAL", "SPATIAL"], ["TEMPORAL", "ELEVATION"], ["SPATIAL", "ELEVATION"]]
WEIGHTS = [1.0, 1.0, 1.0, 0.5, 0.5, 0.5]
P_FULL, P_PARTIAL = 0.3, 0.7


def literal(aux, masks):
    """Leg a: the reference's loop on device tensors, in place on its arguments (the caller passes clones)"""
    B = aux.size(0)
    full = torch.rand(B, device=aux.device) < P_FULL
    aux[full] = 0.0
    masks[full] = False
    u = torch.rand(B, device=aux.device)
    for i in range(B):
        if not full[i]:
            if u[i] < P_PARTIAL:
                combo = random.choices(WHITELIST, weights=WEIGHTS, k=1)[0]
                a, m = aux[i].clone(), masks[i].clone()
                for comp in combo:
                    s, e = BOUNDS[comp]
                    a[s:e] = 0.0
                    m[s:e] = False
                aux[i] = a
                masks[i] = m
    masks = masks.contiguous().clone()
    stats = {c: (masks[:, s:e].all(dim=1).sum().item() / B) * 100.0 for c, (s, e) in BOUNDS.items()}
    return aux, masks, stats


def batched_tables(device):
    total = sum(WEIGHTS)
    acc, thr = 0.0, []
    for w in WEIGHTS:
        acc += w
        thr.append(acc / total)
    thr[-1] = 1.0
    cols = torch.zeros(len(WHITELIST), 15, dtype=torch.bool)
    for k, combo in enumerate(WHITELIST):
        for comp in combo:
            cols[k, BOUNDS[comp][0]:BOUNDS[comp][1]] = True
    return torch.tensor(thr, dtype=torch.float32, device=device), cols.to(device)


def batched(aux, masks, thr, cols):
    """Leg b: batched torch ops, no host read"""
    B = aux.size(0)
    u = torch.rand(3, B, device=aux.device)
    full = u[0] < P_FULL
    partial = ~full & (u[1] < P_PARTIAL)
    k = torch.searchsorted(thr, u[2], right=True).clamp_(max=thr.numel() - 1)
    clear = full[:, None] | (partial[:, None] & cols[k])
    aux = torch.where(clear, torch.zeros((), device=aux.device), aux)
    masks = masks & ~clear
    stats = torch.stack([masks[:, s:e].all(dim=1).sum() for s, e in BOUNDS.values()]).to(torch.float64) / B * 100.0
    return aux, masks, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--iters-a", type=int, default=20, help="timed batches of the literal leg a (hundreds of host reads per batch)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_meta_mask.py needs the MI355X: there is no CPU path")
    from linnaeus_amd import GPUMetaMasking

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(42)
    random.seed(42)
    B = args.batch
    aux0 = torch.randn(B, 15, device=dev)
    masks0 = torch.rand(B, 15, device=dev) < 0.95
    thr, cols = batched_tables(dev)
    masker = GPUMetaMasking(BOUNDS, whitelist=WHITELIST, weights=WEIGHTS)
    kw = dict(p_full=P_FULL, partial_enabled=True, p_partial=P_PARTIAL)

    def leg(name, n):
        for _ in range(n):
            if name == "a":
                literal(aux0.clone(), masks0.clone())
            elif name == "b":
                batched(aux0.clone(), masks0.clone(), thr, cols)
            else:
                aux0.clone(), masks0.clone()  # the kernel leaves its inputs alone; cloned all the same, like the other legs
                _, m = masker(aux0, masks0, **kw)
                masker.stats(m)

    names = ("a", "b", "c")
    iters = {"a": args.iters_a, "b": args.iters, "c": args.iters}
    rows = {k: [] for k in names}
    for name in names:
        leg(name, 2 if name == "a" else args.warmup)
    torch.cuda.synchronize()
    for r in range(args.repeats):
        for name in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            leg(name, iters[name])
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / iters[name] * 1e6
            rows[name].append(round(us, 2))
            print(f"[bench_meta_mask] repeat {r} leg {name}: {us:.2f} us / batch over {iters[name]} batches", file=sys.stderr, flush=True)

    # the same draws give the same result in legs b and c (leg a's pick comes from Python's random stream and is not comparable)
    draws = torch.rand(3, B, device=dev)
    masker._inject = {"draws": draws}
    ca, cm = masker(aux0, masks0, **kw)
    cs = masker.stats(cm)
    masker._inject = None
    full = draws[0] < P_FULL
    partial = ~full & (draws[1] < P_PARTIAL)
    k = torch.searchsorted(thr, draws[2], right=True).clamp_(max=thr.numel() - 1)
    clear = full[:, None] | (partial[:, None] & cols[k])
    agree = bool(torch.equal(ca, torch.where(clear, torch.zeros((), device=dev), aux0)) and torch.equal(cm, masks0 & ~clear))
    agree = agree and bool(torch.equal(cs, torch.stack([cm[:, s:e].all(dim=1).sum() for s, e in BOUNDS.values()]).to(torch.float64) / B * 100.0))

    bd, cb, ct = masker._tables(dev)
    from linnaeus_amd import collate as K

    mk = masks0.view(torch.uint8)
    oa, om = torch.empty_like(aux0), torch.empty_like(mk)
    counts = torch.zeros(5, dtype=torch.int32, device=dev)

    def launches(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            K._meta_mask_launch(aux0, mk, oa, om, B, 15, bd, 3, tables=(cb, ct), draws=draws, p_full=P_FULL, p_partial=P_PARTIAL, partial_on=True, counts=counts)
            K._meta_mask_launch(None, om, None, None, B, 15, bd, 3, counts=counts)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    launches(20)
    pair_us = launches(500)
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    print(json.dumps({
        "workload": f"metadata masking + component statistics of one batch, B {B}, D 15 (2 + 3 + 10), p_full {P_FULL}, p_partial {P_PARTIAL}, six weighted "
                    f"combinations; {args.warmup} warm-up + {args.iters} timed batches per leg ({args.iters_a} for leg a), {args.repeats} alternated repeats, "
                    "median, host wall clock between device synchronisations",
        "a_reference_loop_on_device_tensors_us": med["a"], "b_batched_torch_ops_us": med["b"], "c_gpu_meta_masking_us": med["c"],
        "a_over_c": round(med["a"] / med["c"], 2), "b_over_c": round(med["b"] / med["c"], 2),
        "c_two_launches_enqueued_back_to_back_us": round(pair_us, 3), "all_repeats_us": rows, "iters_leg_a": args.iters_a,
        "legs_b_and_c_agree_on_the_same_draws": agree, "bytes_per_batch": B * 15 * (4 + 1) * 2}), flush=True)


if __name__ == "__main__":
    main()
