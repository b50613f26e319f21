"""The optimizer step of a configured run, clip included: `build_optimizer`'s fused step against the best the package offered before it.

    python tools/bench_optim_step.py [--steps 50] [--warmup 10] [--repeats 7] [--log profiles/optim_build_bench.log]
                                     [--guard] [--other-lib PATH]

Parameters: mFormerV1_sm with four heads (shapes and names from the model built on the CPU), seeded values and gradients on the device,
TRAIN.CLIP_GRAD 5.0 with a gradient norm above it.  Two jobs:

  muon   OPTIMIZER.NAME = muon.  `fused`: FusedMultiOptimizer.step() (one norm pass for all gradients, FusedMuon + FusedAdamW clipping
         by it) and grad_norms() as device scalars.  `fused+read`: the same, then the three norms read to the host in one copy.
         `before`: the block of train.py:279-313 as a user had to write it -- clip_grad_norm_(inf) and its .item(),
         clip_grad_norm_(5.0) and its .item() -- then FusedMuon.step() and FusedAdamW.step().
  sgd    OPTIMIZER.NAME = sgd.  `fused`: FusedSGD.step() with its own clip; `before`: the same two clip passes, then torch.optim.SGD.step().

--guard adds the non-finite guard to both jobs: `guard` is `fused` built with nonfinite_guard=True (the same launches; every workgroup
reads the skip flag first), `noclip` and `guard-noclip` the step without a clip, guard off and on (the guard forces the norm pass: two
more launches).  --other-lib PATH adds `other`: `fused` on a second optimizer whose calls go to the library at PATH, e.g. one built from
the parent commit, so two builds alternate in one process on one device.

The candidates of a job run in this process on the same device and alternate round by round (`--repeats` rounds); a round times
`--steps` steps between two device events after `--warmup` untimed ones.  Reported: median and range of the rounds in microseconds
per step, and launches per step where the library counts them.  Last line: one JSON object; the log file gets the same text.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from linnaeus_amd import _lib as L  # noqa: E402
from linnaeus_amd.config import ConfigNode  # noqa: E402
from linnaeus_amd.optim import FusedAdamW, FusedMuon, build_optimizer, set_weight_decay  # noqa: E402

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
CLIP = 5.0


class Named(torch.nn.Module):
    """the model as build_optimizer sees it: named parameters (on the device)"""

    def __init__(self, named):
        super().__init__()
        self._named = named

    def named_parameters(self, *a, **k):
        return iter(self._named)

    def parameters(self, *a, **k):
        return (p for _, p in self._named)


def sm_named(gen):
    from linnaeus_amd import arch_config, build_model

    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = [t for t, _ in TASKS]
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in TASKS}
    shapes = [(n, tuple(p.shape)) for n, p in build_model(cfg, num_classes=dict(TASKS)).named_parameters()]
    named = [(n, torch.nn.Parameter(torch.randn(*s, device="cuda", generator=gen) * 0.02)) for n, s in shapes]
    for _, p in named:
        p.grad = torch.randn(p.shape, device="cuda", generator=gen) * 1e-2
    return Named(named)


def config(name):
    return ConfigNode({"OPTIMIZER": {"NAME": name}, "LR_SCHEDULER": {"BASE_LR": 1e-4}, "TRAIN": {"CLIP_GRAD": CLIP}})


def clip_block(params):
    """train.py:282-297"""
    pre = torch.nn.utils.clip_grad_norm_(params, float("inf")).item()
    returned = torch.nn.utils.clip_grad_norm_(params, CLIP).item()
    return pre, returned


def window(step, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps  # microseconds per step


def through(lib, step):
    """`step` with every library call of linnaeus_amd going to `lib`"""

    def run():
        mine, L._lib = L._lib, lib
        try:
            return step()
        finally:
            L._lib = mine

    run.lib = lib
    return run


def load_other(path):
    """a second build of the library, with the argument types of the entry points an optimizer step calls"""
    lib, mine = C.CDLL(path), L.lib()
    for name in ("lnx_sgd_step", "lnx_ademamix_step", "lnx_muon_step", "lnx_muon_layout"):
        getattr(lib, name).argtypes = getattr(mine, name).argtypes
    lib.lnx_last_error.restype = C.c_char_p
    lib.lnx_optim_launches.restype = lib.lnx_muon_launches.restype = C.c_int64
    return lib


def launches(step):
    lib = getattr(step, "lib", None) or L.lib()
    torch.cuda.synchronize()
    o, m = lib.lnx_optim_launches(), lib.lnx_muon_launches()
    step()
    torch.cuda.synchronize()
    return lib.lnx_optim_launches() - o + lib.lnx_muon_launches() - m


def run_job(candidates, args, say):
    for step in candidates.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    times = {k: [] for k in candidates}
    for _ in range(args.repeats):
        for k, step in candidates.items():
            times[k].append(window(step, args.steps))
    out = {}
    for k, v in times.items():
        out[k] = {"us_median": round(statistics.median(v), 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1), "lnx_launches": launches(candidates[k])}
        say(f"  {k:11s} {out[k]['us_median']:9.1f} us/step  (rounds {out[k]['us_min']:.1f} .. {out[k]['us_max']:.1f})   {out[k]['lnx_launches']:3d} launches of the library per step")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--log", default=os.path.join(REPO, "profiles", "optim_build_bench.log"))
    ap.add_argument("--guard", action="store_true", help="add the rows of the non-finite guard")
    ap.add_argument("--other-lib", default=None, help="a second build of liblnx_hip.so: adds the row `other`")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_optim_step.py measures on the GPU; there is none here")
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "repeats": args.repeats, "clip": CLIP}
    other = None
    if args.other_lib:
        other = load_other(args.other_lib)
        res["lnx_version"], res["other_lnx_version"] = L.lib().lnx_version(), other.lnx_version()
        say(f"library version {res['lnx_version']}; other library {args.other_lib}: version {res['other_lnx_version']}")

    def extra_rows(name):
        """the rows of --guard and --other-lib for OPTIMIZER.NAME = name, each on parameters of its own"""
        rows, keep = {}, []

        def row(key, wrap=lambda f: f, **kw):
            model = fresh()
            opt = build_optimizer(config(name), model, **kw)
            keep.append((model, opt))
            rows[key] = wrap(opt.step)

        if other is not None:
            row("other", lambda f: through(other, f))
        if args.guard:
            row("guard", nonfinite_guard=True)
            row("noclip", max_grad_norm=None)
            row("guard-noclip", max_grad_norm=None, nonfinite_guard=True)
        return rows, keep

    def fresh():
        gen.manual_seed(0)
        return sm_named(gen)

    # ---- muon
    a, b = fresh(), fresh()
    n_params = sum(p.numel() for p in a.parameters())
    norm = float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in a.parameters())))
    say(f"device {res['device']}; mFormerV1_sm: {len(list(a.parameters()))} tensors, {n_params / 1e6:.2f} M parameters, gradient norm {norm:.1f}, clip {CLIP}; "
        f"{args.repeats} rounds of {args.steps} steps after {args.warmup}")
    multi = build_optimizer(config("muon"), a)
    ref = build_optimizer(config("muon"), b, max_grad_norm=None)  # the same split, no clip: what the parent offered
    assert type(ref.optimizers["MUON"]) is FusedMuon and type(ref.optimizers["ADAMW"]) is FusedAdamW
    b_params = list(b.parameters())

    def fused():
        multi.step()
        return multi.grad_norms()

    def fused_read():
        multi.step()
        return torch.stack(multi.grad_norms()).tolist()

    def before():
        clip_block(b_params)
        ref.optimizers["MUON"].step()
        ref.optimizers["ADAMW"].step()

    say(f"muon: {len(multi.optimizers['MUON'].param_groups[0]['params'])} matrices to FusedMuon, {len(multi.optimizers['ADAMW'].param_groups[0]['params'])} tensors to FusedAdamW")
    rows, keep = extra_rows("muon")
    res["muon"] = run_job({"fused": fused, "fused+read": fused_read, "before": before, **rows}, args, say)
    res["muon"]["speedup"] = round(res["muon"]["before"]["us_median"] / res["muon"]["fused"]["us_median"], 3)
    say(f"  before / fused = {res['muon']['speedup']:.3f}x")
    del multi, ref, a, b, b_params, rows, keep
    torch.cuda.empty_cache()

    # ---- sgd
    a, b = fresh(), fresh()
    sgd = build_optimizer(config("sgd"), a)
    b_params = list(b.parameters())
    tsgd = torch.optim.SGD(set_weight_decay(b), lr=1e-4, momentum=0.9, weight_decay=0.05, nesterov=True)

    def before_sgd():
        clip_block(b_params)
        tsgd.step()

    say(f"sgd: {n_params * 20 / 1e6:.0f} MB of update traffic and {n_params * 4 / 1e6:.0f} MB of norm pass per fused step")
    rows, keep = extra_rows("sgd")
    res["sgd"] = run_job({"fused": sgd.step, "before": before_sgd, **rows}, args, say)
    if args.guard:
        say(f"sgd: every guarded step of this run was taken: skipped_steps() = {int(keep[-1][1].skipped_steps())}")
    res["sgd"]["speedup"] = round(res["sgd"]["before"]["us_median"] / res["sgd"]["fused"]["us_median"], 3)
    res["sgd"]["fused_GBps"] = round(n_params * 24 / (res["sgd"]["fused"]["us_median"] * 1e-6) / 1e9, 1)
    say(f"  before / fused = {res['sgd']['speedup']:.3f}x; fused step moves {n_params * 24 / 1e6:.0f} MB: {res['sgd']['fused_GBps']:.0f} GB/s end to end (launch gaps included)")
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
