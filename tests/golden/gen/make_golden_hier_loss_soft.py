#!/usr/bin/env python3
"""Generate tests/golden/hier_loss_soft.npz from the *reference itself*: weighted_hierarchical_loss
(loss/hierarchical_loss.py:24-406) on [B, C] mixup-style float targets.

Runs only where the reference is mounted (see make_golden.py, whose import recipe and hier_loss case this follows):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen/make_golden_hier_loss_soft.py

The three tasks, the smoothing matrices, the class weights and the task weights are those of hier_loss.npz (read from it); the
logits and the targets are new.  Targets are convex mixes lam * onehot(a) + (1 - lam) * onehot(b) with lam in {0.7, 0.35}: rows
where class 0 holds more than 0.5 (null by the reference's `target[:, 0] > 0.5` test), rows whose tie-free maximum is not the
first column, and rows where class 0 holds mass but less than 0.5 (not null).  Recorded: the four deterministic masking modes with
class weights.  Nothing from the reference is copied: the fixture holds numbers only.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path[:0] = [os.path.join(HERE, "_stubs"), "/root/reference", REPO]
sys.dont_write_bytecode = True

import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

warnings.filterwarnings("ignore")
logging.disable(logging.CRITICAL)

from linnaeus.config import get_default_config  # noqa: E402
from linnaeus.loss.gradient_weighting import GradientWeighting  # noqa: E402
from linnaeus.loss.hierarchical_loss import weighted_hierarchical_loss  # noqa: E402
from linnaeus.loss.taxonomy_label_smoothing import TaxonomyAwareLabelSmoothingCE  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SEED = 20251003
MODES = (("sched1", 1.0, False, False), ("sched0", 0.0, False, False), ("phase1", 1.0, True, False), ("val", 0.0, False, True))


class Sched:  # the one method the loss path calls (ops_schedule/ops_schedule.py:655)
    def __init__(self, p):
        self.p = p

    def get_null_mask_prob(self, step):
        return self.p


def main():
    z = np.load(os.path.join(OUT, "hier_loss.npz"))
    tasks = [str(t) for t in z["tasks"]]
    classes = [int(c) for c in z["classes"]]
    g = torch.Generator().manual_seed(SEED + 29)
    B = 16
    rec = {"tasks": z["tasks"], "classes": z["classes"], "task_weights": z["task_weights"]}
    logits, targets, soft, cw = {}, {}, {}, {}
    for t, c in zip(tasks, classes):
        logits[t] = (torch.randn(B, c, generator=g) * 2).requires_grad_(True)
        a = torch.randint(1, c, (B,), generator=g)
        b = torch.randint(1, c, (B,), generator=g)
        a[:4] = 0                       # rows 0..3: class 0 holds lam = 0.7 -> null
        b[4:7] = 0                      # rows 4..6: class 0 holds 0.3 or 0.65 -> null only where lam = 0.35
        lam = torch.where(torch.arange(B) % 2 == 0, torch.tensor(0.7), torch.tensor(0.35))
        same = a == b
        b = torch.where(same, (b % (c - 1)) + 1 if c > 2 else b, b)  # keep the two classes distinct: the maximum is tie-free
        y = torch.zeros(B, c)
        y[torch.arange(B), a] += lam
        y[torch.arange(B), b] += 1.0 - lam
        top = y.max(1).values
        assert ((y == top[:, None]).sum(1) == 1).all(), "a target row has a tied maximum"
        targets[t] = y
        soft[t] = torch.from_numpy(z[f"soft_{t}"])
        cw[t] = {i: float(z[f"cw_{t}"][i]) for i in range(0, c, 2)}  # the sparse dict of hier_loss.npz: missing -> 1.0
        rec[f"logits_{t}"] = logits[t].detach().numpy()
        rec[f"target_{t}"] = y.numpy()
        rec[f"soft_{t}"] = z[f"soft_{t}"]
        rec[f"cw_{t}"] = z[f"cw_{t}"]
        n_null = int((y[:, 0] > 0.5).sum())
        n_late = int((y.argmax(1) != 0).sum())
        print(f"[hier_loss_soft] {t}: {n_null} null rows, {n_late} rows whose maximum is not column 0")
        assert 0 < n_null < B and n_late > 0
    tw = {t: float(w) for t, w in zip(tasks, z["task_weights"])}
    criteria = {t: TaxonomyAwareLabelSmoothingCE(soft[t]) for t in tasks}
    for mode, prob, phase1, val in MODES:
        cfg = get_default_config()
        cfg.defrost()
        cfg.TRAIN.PHASE1_MASK_NULL_LOSS = phase1
        gw = GradientWeighting(tasks, cfg, "static", init_weights=tw, class_weights=cw)
        for t in tasks:
            logits[t].grad = None
        total, comps, _ = weighted_hierarchical_loss({t: logits[t] for t in tasks}, targets, criteria, gw, Sched(prob), 10, is_validation=val, config=cfg)
        total.backward()
        rec[f"{mode}_total"] = np.float64(total.item())
        rec[f"{mode}_weighted"] = np.array([comps["weighted_tasks"][t] for t in tasks])
        rec[f"{mode}_masked_mean"] = np.array([comps["masked_tasks"][t] for t in tasks])
        rec[f"{mode}_raw_mean"] = np.array([comps["tasks"][t] for t in tasks])
        for t in tasks:
            rec[f"{mode}_grad_{t}"] = logits[t].grad.numpy().copy()
        print(f"[hier_loss_soft/{mode}] total {total.item():.6f} weighted {rec[f'{mode}_weighted']}")
    np.savez_compressed(os.path.join(OUT, "hier_loss_soft.npz"), **rec)


if __name__ == "__main__":
    main()
