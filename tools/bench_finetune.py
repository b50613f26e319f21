"""Fine-tuning steps of mFormerV1_sm with a frozen prefix against the same freeze state on the full training plan.

    python tools/bench_finetune.py [--batch 256] [--steps 10] [--warmup 5] [--repeats 7] [--log profiles/finetune_bench.log]

One step = forward + probe loss + backward (bf16, DropPath as configured, direct gradient mode).  Four freeze states: everything trains,
the conv trunk frozen (cut `tokens_1`), `unfreeze_last_blocks(2)`, heads only.  Each state runs on two models that share nothing but the
process and the device: one whose plans are created with the frozen prefix on, one created with LNX_FROZEN_PREFIX=0 -- the full
training plan for the same `requires_grad` state, which is what the package ran before the planner knew about frozen units.  The two
alternate round by round (`--repeats` rounds of `--steps` steps between two device events, after `--warmup` untimed steps); reported
are the median and the range of the rounds in milliseconds per step and the workspace bytes of each plan.  Last line: one JSON object;
the log file gets the same text.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TASKS = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
STATES = (("all trainable", lambda m: m.freeze_through("stem")),
          ("conv trunk frozen (cut tokens_1)", lambda m: m.freeze_through("tokens_1")),
          ("unfreeze_last_blocks(2)", lambda m: m.unfreeze_last_blocks(2)),
          ("heads only", lambda m: m.freeze_through("heads")))


def make_model():
    from linnaeus_amd import arch_config, build_model

    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = [t for t, _ in TASKS]
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in TASKS}
    torch.manual_seed(0)
    model = build_model(cfg, num_classes=dict(TASKS)).cuda().train()
    model.set_compute_dtype("bf16")
    model.grad_mode = "direct"
    return model


def window(step, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps  # milliseconds per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    models = {"on": make_model(), "off": make_model()}
    B = a.batch
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, 3, 224, 224, device="cuda", generator=g)
    meta = torch.randn(B, sum(models["on"].meta_dims), device="cuda", generator=g) if models["on"].meta_dims else None

    def stepper(model):
        def step():
            out = model(x, meta)
            sum(v.float().square().mean() for v in out.values()).backward()
        return step

    result = {"batch": B, "states": {}}
    say(f"mFormerV1_sm bf16 batch {B}: forward + probe loss + backward, ms per step (median [min .. max] of {a.repeats} rounds of {a.steps} steps)")
    for name, freeze in STATES:
        steps = {}
        ws = {}
        for which, model in models.items():
            freeze(model)
            model.zero_grad(set_to_none=True)
            # the switch is read when a plan is created: the first forward of this freeze state on this model
            if which == "off":
                os.environ["LNX_FROZEN_PREFIX"] = "0"
            else:
                os.environ.pop("LNX_FROZEN_PREFIX", None)
            steps[which] = stepper(model)
            ws[which] = model.workspace_bytes(B, 224)
            for _ in range(a.warmup):
                steps[which]()
            torch.cuda.synchronize()
        os.environ.pop("LNX_FROZEN_PREFIX", None)
        rounds = {"on": [], "off": []}
        for _ in range(a.repeats):
            for which in ("on", "off"):
                rounds[which].append(window(steps[which], a.steps))
        rep = models["on"].trainable_report(B, 224)
        entry = {"cut": rep["cut"], "backward_units": rep["backward_units"]}
        for which in ("on", "off"):
            r = rounds[which]
            entry[which] = {"ms": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3), "workspace_bytes": ws[which]}
        result["states"][name] = entry
        say(f"  {name:34s} cut {rep['cut']:12s} units {rep['backward_units']:2d} | frozen prefix on: {entry['on']['ms']:7.3f} [{entry['on']['min']:.3f} .. "
            f"{entry['on']['max']:.3f}] ws {ws['on'] / 2**20:8.1f} MiB | LNX_FROZEN_PREFIX=0: {entry['off']['ms']:7.3f} [{entry['off']['min']:.3f} .. "
            f"{entry['off']['max']:.3f}] ws {ws['off'] / 2**20:8.1f} MiB")
        for model in models.values():
            model.release_plans()
    say(json.dumps(result))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
