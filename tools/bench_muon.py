"""Muon.step() (a Python loop over parameters: ~50 launches each) against FusedMuon.step() (3 * ns_steps + 3 launches for all of them)
on the parameters optimizers/build.py:130-154 hands to Muon for mFormerV1_sm: the 52 2-D / 4-D tensors whose names hold no 'embed',
'token', 'head' or 'classifier'.

    python tools/bench_muon.py [--steps 10] [--warmup 3] [--log profiles/muon_bench.log]

Seeded parameters and gradients, both optimizers in this process on the same device, timed between device events after warm-up.
Per optimizer: launches per step, milliseconds per step, and the rate of the Newton-Schulz part -- the step's time minus the time
of the same step with ns_steps = 0 -- against the algorithmic ns_steps * (4 m^2 n + 2 m^3) FLOP per matrix (m <= n its two sides).
FusedMuon's launches are lnx_muon_launches(); Muon's are its lnx_gemm_nt launches plus the torch operators it dispatches, views
excluded (each of those is at least one launch).  Last line: one JSON object with every number; the log file gets the same text.

    python tools/bench_muon.py --world 1 2 4 8 [--steps 50] [--log profiles/muon_sharded_bench.log]

times ShardedFusedMuon instead: for each world size W and each rank r < W, in this one process on this one device, that rank's
begin_step + finish_step -- the norm-free local work: lnx_muon_orthogonalize over the matrices rank r owns, then lnx_muon_apply_packed over
all 52 -- with a no-op `gather` seam and a gathered buffer that is already there (the peers' segments hold zeros; the time does not
depend on the values).  Reported per W: every rank's milliseconds, their maximum, launches and workspace bytes per rank, the partition's
max / mean cost, and FusedMuon.step timed in the same run, before and after the sharded runs.  The collective itself is NOT timed: no
run of this project has had more than one device.
"""
import argparse
import json
import math
import os
import sys

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linnaeus_amd import _lib as L  # noqa: E402
from linnaeus_amd.optim import FusedMuon, Muon, ShardedFusedMuon, muon_parameters  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
HYPER = dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True)
VIEWS = ("aten.t.", "aten.view.", "aten.slice.", "aten.detach.", "aten.alias.", "aten._unsafe_view.", "aten.transpose.", "aten.as_strided.", "aten.expand.")


def sm_muon_shapes():
    from linnaeus_amd import arch_config, build_model

    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = [t for t, _ in TASKS]
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in TASKS}
    return [tuple(p.shape) for p in muon_parameters(build_model(cfg, num_classes=dict(TASKS)))]


class CountOps(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if not str(func).startswith(VIEWS):
            self.n += 1
        return func(*args, **(kwargs or {}))


def gemm_launches():
    return sum(L.lib().lnx_nt_kernel_launches(k) for k in range(16))


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
    return e0.elapsed_time(e1) / steps  # ms per step


def sharded(args, shapes, say):
    """--world: every rank's local work at every world size, and FusedMuon.step around them; returns the result object"""
    dev = torch.cuda.get_device_name(0)
    nparam = sum(math.prod(s) for s in shapes)
    say(f"device {dev}, one device, one process; mFormerV1_sm Muon set: {len(shapes)} tensors, {nparam / 1e6:.2f} M parameters, ns_steps = {args.ns_steps}; "
        f"{args.steps} timed steps after {args.warmup} warm-up steps per figure; the collective is not timed (no-op gather seam)")
    gen = torch.Generator(device="cuda").manual_seed(0)
    init = [torch.randn(*s, device="cuda", generator=gen) * 0.02 for s in shapes]
    grads = [torch.randn(*s, device="cuda", generator=gen) * 1e-3 for s in shapes]
    res = {"device": dev, "tensors": len(shapes), "params": nparam, "ns_steps": args.ns_steps, "steps": args.steps, "worlds": {}}

    def measure(make):
        params = [torch.nn.Parameter(t.clone()) for t in init]
        for p, g in zip(params, grads):
            p.grad = g
        opt = make(params)
        ms = timed(opt.step, args.steps, args.warmup)
        before = L.lib().lnx_muon_launches()
        opt.step()
        torch.cuda.synchronize()
        out = (ms, L.lib().lnx_muon_launches() - before, opt.workspace_bytes(), opt)
        return out

    def fused():
        ms, launches, ws, _ = measure(lambda ps: FusedMuon(ps, ns_steps=args.ns_steps, **HYPER))
        torch.cuda.empty_cache()
        return ms, launches, ws

    f0 = fused()
    say(f"FusedMuon.step (before)   {f0[0]:8.3f} ms  {f0[1]} launches  workspace {f0[2]} bytes")
    for world in args.world:
        ranks = []
        for r in range(world):
            ms, launches, ws, opt = measure(lambda ps: ShardedFusedMuon(ps, ns_steps=args.ns_steps, rank=r, world_size=world, gather=lambda out, seg: None, **HYPER))
            rep = opt.partition_report()
            ranks.append({"rank": r, "ms": round(ms, 3), "launches": launches, "workspace_bytes": ws, "owned": rep["owner"].count(r),
                          "momentum_bytes": 4 * sum(p.numel() for p in opt.state)})
            del opt
            torch.cuda.empty_cache()
        worst = max(x["ms"] for x in ranks)
        res["worlds"][str(world)] = {"ranks": ranks, "max_ms": worst, "max_over_mean_cost": round(rep["max_over_mean"], 4), "seg_elems": rep["seg_elems"],
                                     "gathered_bytes": rep["gathered_bytes"]}
        say(f"world {world}: max / mean cost {rep['max_over_mean']:.4f}, seg_elems {rep['seg_elems']}, gathered buffer {rep['gathered_bytes']} bytes")
        for x in ranks:
            say(f"    rank {x['rank']}: {x['ms']:8.3f} ms  {x['launches']} launches  {x['owned']:2d} matrices  workspace {x['workspace_bytes']} bytes  "
                f"momentum {x['momentum_bytes']} bytes")
        say(f"    rank maximum {worst:.3f} ms")
    f1 = fused()
    say(f"FusedMuon.step (after)    {f1[0]:8.3f} ms  {f1[1]} launches  workspace {f1[2]} bytes")
    base = min(f0[0], f1[0])  # the comparison least kind to the sharded step
    res["fused_muon"] = {"ms_before": round(f0[0], 3), "ms_after": round(f1[0], 3), "launches": f0[1], "workspace_bytes": f0[2]}
    for world, w in res["worlds"].items():
        w["max_over_fused"] = round(w["max_ms"] / base, 3)
        say(f"world {world}: rank maximum / FusedMuon.step = {w['max_over_fused']:.3f}  (an even split of the whole step would give {1 / int(world):.3f})")
    say("what is not divided by the world size: the apply launch, which runs over all matrices on every rank, and the launch count -- a rank "
        "makes the same 3 * ns_steps + 4 launches over ever smaller grids")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=None, help="timed steps per figure (default 10; 50 with --world)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns-steps", type=int, default=5)
    ap.add_argument("--world", type=int, nargs="+", default=None, help="time ShardedFusedMuon's per-rank local work at these world sizes instead")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    profiles = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    if args.log is None:
        args.log = os.path.join(profiles, "muon_bench.log" if args.world is None else "muon_sharded_bench.log")
    if args.steps is None:
        args.steps = 10 if args.world is None else 50
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    shapes = sm_muon_shapes()
    if args.world is not None:
        if not torch.cuda.is_available():
            raise SystemExit("tools/bench_muon.py needs a GPU")
        if any(w < 1 for w in args.world):
            raise SystemExit("--world: world sizes start at 1")
        say(json.dumps(sharded(args, shapes, say)))
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    flop = 0
    for s in shapes:
        rows, cols = s[0], math.prod(s[1:])
        m, n = min(rows, cols), max(rows, cols)
        flop += args.ns_steps * (4 * m * m * n + 2 * m ** 3)
    nparam = sum(math.prod(s) for s in shapes)
    say(f"device {torch.cuda.get_device_name(0)}; mFormerV1_sm Muon set: {len(shapes)} tensors, {nparam / 1e6:.2f} M parameters, "
        f"{flop / 1e9:.1f} GFLOP of Newton-Schulz per step at ns_steps = {args.ns_steps}")
    gen = torch.Generator(device="cuda").manual_seed(0)
    init = [torch.randn(*s, device="cuda", generator=gen) * 0.02 for s in shapes]
    grads = [torch.randn(*s, device="cuda", generator=gen) * 1e-3 for s in shapes]
    res = {"device": torch.cuda.get_device_name(0), "tensors": len(shapes), "params": nparam, "ns_gflop": round(flop / 1e9, 2), "ns_steps": args.ns_steps}
    for name, cls in (("muon", Muon), ("fused_muon", FusedMuon)):
        ms = {}
        for ns in (args.ns_steps, 0):
            params = [torch.nn.Parameter(t.clone()) for t in init]
            opt = cls(params, ns_steps=ns, **HYPER)

            def step():
                for p, g in zip(params, grads):  # (Muon lerps .grad in place, so the values drift from step to step; the time does not depend on them)
                    p.grad = g
                opt.step()

            ms[ns] = timed(step, args.steps, args.warmup)
            if ns == args.ns_steps:
                g0, f0 = gemm_launches(), L.lib().lnx_muon_launches()
                with CountOps() as ops:
                    step()
                torch.cuda.synchronize()
                launches = (L.lib().lnx_muon_launches() - f0) if cls is FusedMuon else (gemm_launches() - g0) + ops.n
                if cls is FusedMuon:
                    res["workspace_bytes"] = opt.workspace_bytes()
            del opt, params
            torch.cuda.empty_cache()
        ns_ms = ms[args.ns_steps] - ms[0]
        rate = flop / (ns_ms * 1e-3) / 1e12 if ns_ms > 0 else float("nan")
        res[name] = {"launches": launches, "ms": round(ms[args.ns_steps], 3), "ms_ns0": round(ms[0], 3), "ns_tflops": round(rate, 1)}
        say(f"{name:11s} {launches:5d} launches/step  {ms[args.ns_steps]:9.3f} ms/step  ({ms[0]:.3f} ms at ns_steps = 0; Newton-Schulz part {ns_ms:.3f} ms = {rate:.1f} TFLOP/s)")
    res["speedup"] = round(res["muon"]["ms"] / res["fused_muon"]["ms"], 2)
    say(f"Muon.step / FusedMuon.step = {res['speedup']:.2f}x; FusedMuon workspace {res['workspace_bytes']} bytes = {res['workspace_bytes'] / nparam:.2f} per parameter")
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
