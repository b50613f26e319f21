#!/usr/bin/env python3
"""Generate tests/golden/ademamix.npz from the reference's own AdEMAMix (linnaeus/optimizers/ademamix.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_ademamix.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/, runs six optimizer steps on CPU
and writes numbers only: the initial parameters, every step's gradients, the parameters after every step, and the
optimizer state after steps 3 and 6.  Gradients and initial parameters are rounded to bf16-representable fp32 values
(exact inputs either way; it keeps the file small).

Parameters p0..p5 of shapes SHAPES; two groups:
  group 0 = p0..p2: lr 3e-3 (1e-3 from step 4 on), weight_decay 0.05, betas (0.9, 0.999, 0.9999), alpha 5, T None
  group 1 = p3..p5: lr 1e-2, weight_decay 0, betas (0.8, 0.95, 0.999), alpha 2, T 4 (the schedule runs past T)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "optimizers", "ademamix.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
sys.path[:0] = [os.path.join(HERE, "_stubs"), os.path.abspath(sys.argv[1])]
sys.dont_write_bytecode = True

import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

warnings.filterwarnings("ignore")
logging.disable(logging.CRITICAL)

from linnaeus.optimizers.ademamix import AdEMAMix  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "ademamix.npz")
SEED = 20251016
SHAPES = [(49, 37), (5,), (1029,), (3, 3, 7, 7), (1,), (4099,)]
STEPS = 6
GROUP0_LR = [3e-3, 3e-3, 3e-3, 1e-3, 1e-3, 1e-3]
STATE_KEYS = ("exp_avg", "exp_avg_sq", "exp_avg_slow")


def bf16_exact(t):
    return t.to(torch.bfloat16).float()


def main():
    torch.manual_seed(SEED)
    gen = torch.Generator().manual_seed(SEED)
    params = [torch.nn.Parameter(bf16_exact(torch.randn(*s, generator=gen))) for s in SHAPES]
    rec = {"shapes": np.array([str(s) for s in SHAPES]), "group0_lr": np.array(GROUP0_LR, dtype=np.float64)}
    for i, p in enumerate(params):
        rec[f"p{i}_init"] = p.detach().numpy().copy()
    opt = AdEMAMix([{"params": params[:3], "lr": GROUP0_LR[0], "weight_decay": 0.05},
                    {"params": params[3:], "lr": 1e-2, "weight_decay": 0.0, "betas": (0.8, 0.95, 0.999), "alpha": 2.0, "T_alpha_beta3": 4}],
                   lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0, alpha=5.0, T_alpha_beta3=None)
    for s in range(STEPS):
        opt.param_groups[0]["lr"] = GROUP0_LR[s]
        for i, p in enumerate(params):
            g = bf16_exact(torch.randn(p.shape, generator=gen) * (0.05 + 0.3 * s) * (1.0 + i))
            p.grad = g
            rec[f"p{i}_grad{s}"] = g.numpy().copy()
        opt.step()
        for i, p in enumerate(params):
            rec[f"p{i}_after{s}"] = p.detach().numpy().copy()
        if s + 1 in (3, STEPS):
            for i, p in enumerate(params):
                st = opt.state[p]
                rec[f"p{i}_step_s{s + 1}"] = np.array(int(st["step"]))
                for k in STATE_KEYS:
                    rec[f"p{i}_{k}_s{s + 1}"] = st[k].numpy().copy()
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
