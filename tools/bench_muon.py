"""Muon.step() (a Python loop over parameters: ~50 launches each) against FusedMuon.step() (3 * ns_steps + 3 launches for all of them)
on the parameters optimizers/build.py:130-154 hands to Muon for mFormerV1_sm: the 52 2-D / 4-D tensors whose names hold no 'embed',
'token', 'head' or 'classifier'.

    python tools/bench_muon.py [--steps 10] [--warmup 3] [--log profiles/muon_bench.log]

Seeded parameters and gradients, both optimizers in this process on the same device, timed between device events after warm-up.
Per optimizer: launches per step, milliseconds per step, and the rate of the Newton-Schulz part -- the step's time minus the time
of the same step with ns_steps = 0 -- against the algorithmic ns_steps * (4 m^2 n + 2 m^3) FLOP per matrix (m <= n its two sides).
FusedMuon's launches are lnx_muon_launches(); Muon's are its lnx_gemm_nt launches plus the torch operators it dispatches, views
excluded (each of those is at least one launch).  Last line: one JSON object with every number; the log file gets the same text.
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
from linnaeus_amd.optim import FusedMuon, Muon, muon_parameters  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ns-steps", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "muon_bench.log"))
    args = ap.parse_args()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    shapes = sm_muon_shapes()
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
