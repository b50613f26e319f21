#!/usr/bin/env python3
"""What turning logits into predictions costs around the eval forward of mFormerV1_sm (batch 512, bf16, 224 px, four tasks of
1000 / 300 / 80 / 20 classes, top 5, hierarchical consistency on).

The `throughput_test` protocol of bench.py --eval (eval mode, no_grad, resident uniform-random inputs, warm-up calls, then timed calls
between two device synchronisations), four legs in ONE process, alternated `--repeats` times so that drift hits all of them alike:

  a   forward only
  b   forward + the reference handler's recipe restated literally (inference/handler.py:186-228): per sample and task torch.softmax,
      torch.topk and two .item() per kept entry, then the consistency walk of inference/postprocessing.py:64-154 in Python.  About
      20 000 host reads per batch: timed over --iters-b batches (stated in the output).
  b2  forward + ONE batched torch.softmax + torch.topk per task, one .cpu() of all of it, the same walk on the host
  c   forward + DevicePredictor.predict_logits (one lnx_predict launch, no host read), one to_results() after the last call, inside
      the timed window

Also: predict_logits alone, enqueued back to back between two events (an upper bound of the kernel's time: launch-rate bound when the
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

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))  # finest first
K = 5
NULL = 0


def make_parents(seed):
    """A seeded forest over TASKS: class 0 of every task is its null and has no parent."""
    g = torch.Generator().manual_seed(seed)
    tabs = {}
    for (child, c), (_, cp) in zip(TASKS[:-1], TASKS[1:]):
        p = torch.randint(1, cp, (c,), generator=g)
        p[0] = -1
        tabs[child] = p
    return tabs


def walk(lists, parents):
    """enforce_hierarchical_consistency for one sample: lists = per task (finest first) [(class, probability), ...]; parents = per task
    a Python list (None for the coarsest).  Returns the final lists, finest first."""
    T = len(lists)
    out = [None] * T
    above = None
    for t in range(T - 1, -1, -1):
        c = lists[t][0][0]
        if t == T - 1:
            out[t], above = lists[t], c
            continue
        if above == NULL or parents[t][c] != above:
            out[t], above = [(NULL, 1.0)], NULL
        else:
            out[t], above = lists[t], c
    return out


def literal(outputs, keys, parents):
    """Leg b: handler.py:186-228 as written -- one softmax, one topk and 2 K .item() per sample and task."""
    B = outputs[keys[0]].shape[0]
    res = []
    for i in range(B):
        lists = []
        for t in keys:
            probs = torch.softmax(outputs[t][i], dim=-1)
            k = min(K, probs.shape[0])
            top_p, top_i = torch.topk(probs, k=k)
            lists.append([(top_i[j].item(), top_p[j].item()) for j in range(k)])
        res.append(walk(lists, parents))
    return res


def batched(outputs, keys, parents):
    """Leg b2: the same results from batched torch ops, ONE device-to-host copy, and the walk on the host."""
    vals, idxs = [], []
    for t in keys:
        p, i = torch.topk(torch.softmax(outputs[t].float(), dim=-1), k=min(K, outputs[t].shape[1]), dim=-1)
        vals.append(p)
        idxs.append(i.to(torch.float64))  # (class indices are exact in double: one tensor, one copy)
    both = torch.cat([torch.cat(vals, 1).double(), torch.cat(idxs, 1)], 1).cpu()
    n = both.shape[1] // 2
    pv, iv = both[:, :n].tolist(), both[:, n:].tolist()
    res = []
    for b in range(len(pv)):
        lists, o = [], 0
        for t in keys:
            k = min(K, outputs[t].shape[1])
            lists.append([(int(iv[b][o + j]), pv[b][o + j]) for j in range(k)])
            o += k
        res.append(walk(lists, parents))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--iters-b", type=int, default=5, help="timed batches of the literal leg b (it takes a large fraction of a second per batch)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"], help="compute dtype of the model")
    ap.add_argument("--logits-dtype", default="fp32", choices=["bf16", "fp32"], help="--kernel-only: storage of the logits (the plan's forward returns fp32)")
    ap.add_argument("--kernel-only", action="store_true", help="only the back-to-back predict loop (for rocprofv3 --kernel-trace --stats)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_predict.py needs the MI355X: there is no CPU path")
    from linnaeus_amd import DevicePredictor, arch_config, build_model

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    torch.manual_seed(42)
    keys = [t for t, _ in TASKS]
    g = torch.Generator(device=dev).manual_seed(42)
    B = args.batch
    tabs = make_parents(42)
    parents_host = [tabs[t].tolist() if t in tabs else None for t in keys]
    dp = DevicePredictor(keys, dict(TASKS), parent_index=tabs, null_index=NULL, top_k=K)

    def predict_loop(outputs, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            dp.predict_logits(outputs)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3  # us per call

    if args.kernel_only:
        dt = torch.bfloat16 if args.logits_dtype == "bf16" else torch.float32
        outputs = {t: torch.randn(B, c, device=dev, generator=g).to(dt) for t, c in TASKS}
        predict_loop(outputs, 20)
        nbytes = sum(v.numel() * v.element_size() for v in outputs.values())
        print(json.dumps({"predict_enqueued_us": round(predict_loop(outputs, 200), 3), "batch": B, "logits_dtype": args.logits_dtype, "logit_bytes": nbytes}), flush=True)
        return

    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = keys
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t in keys}
    model = build_model(cfg, num_classes=dict(TASKS)).to(dev).eval()
    model.set_compute_dtype(args.dtype)
    meta_width = sum(model.meta_dims)
    x = torch.rand(B, 3, 224, 224, device=dev, generator=g)
    meta = torch.rand(B, meta_width, device=dev, generator=g) if meta_width else None

    def leg(name, n):
        pred = None
        for _ in range(n):
            out = model(x, meta)
            if name == "b":
                literal(out, keys, parents_host)
            elif name == "b2":
                batched(out, keys, parents_host)
            elif name == "c":
                pred = dp.predict_logits(out)
        return dp.to_results(pred) if name == "c" else None

    names = ("a", "b", "b2", "c")
    iters = {"a": args.iters, "b": args.iters_b, "b2": args.iters, "c": args.iters}
    rows = {k: [] for k in names}
    with torch.no_grad():
        for name in names:
            leg(name, 1 if name == "b" else args.warmup)
        torch.cuda.synchronize()
        for r in range(args.repeats):
            for name in names:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                leg(name, iters[name])
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) / iters[name] * 1e3
                rows[name].append(round(ms, 4))
                print(f"[bench_predict] repeat {r} leg {name}: {ms:.4f} ms / batch over {iters[name]} batches, {B / ms * 1e3:.0f} img/s", file=sys.stderr, flush=True)
        # the three recipes give the same lists (same outputs every call): classes equal, probabilities to 1e-5
        out = model(x, meta)
        want = batched(out, keys, parents_host)
        lit = literal(out, keys, parents_host)
        got = dp.to_results(dp.predict_logits(out))
        agree = True
        for b in range(B):
            for t, (key, entries) in enumerate(reversed(got[b])):
                for other in (want[b][t], lit[b][t]):
                    agree = agree and [i for i, _ in entries] == [i for i, _ in other] and all(abs(p - q) <= 1e-5 * max(q, 1e-30) + 1e-9 for (_, p), (_, q) in zip(entries, other))
        nullified = sum(len(e) == 1 for s in got for _, e in s)
        pred_us = predict_loop(out, 200)
        nbytes = sum(v.numel() * v.element_size() for v in out.values())
    med = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
    print(json.dumps({
        "workload": f"mFormerV1_sm 3x224x224 eval forward, batch {B}, {args.dtype}, no_grad, 4 tasks 1000/300/80/20, top {K}, consistency on; {args.warmup} warm-up + "
                    f"{args.iters} timed calls per leg ({args.iters_b} for leg b), {args.repeats} alternated repeats, median",
        "a_forward_ms": med["a"], "b_forward_plus_literal_recipe_ms": med["b"], "b2_forward_plus_batched_torch_and_host_walk_ms": med["b2"],
        "c_forward_plus_device_predictor_ms": med["c"],
        "b_minus_a_ms": round(med["b"] - med["a"], 4), "b2_minus_a_ms": round(med["b2"] - med["a"], 4), "c_minus_a_ms": round(med["c"] - med["a"], 4),
        "a_spread_ms": round(max(rows["a"]) - min(rows["a"]), 4), "predict_enqueued_back_to_back_us": round(pred_us, 3),
        "logit_bytes_read_per_batch": nbytes, "logits_dtype": str(out[keys[0]].dtype), "all_repeats_ms": rows, "iters_leg_b": args.iters_b,
        "recipes_agree": bool(agree), "nullified_lists_in_the_check_batch": nullified, "host_reads_per_batch_leg_b": B * len(keys) * 2 * K}), flush=True)


if __name__ == "__main__":
    main()
