#!/usr/bin/env python3
"""Generate tests/golden/basic_loss.npz from the *reference itself*: CrossEntropyLoss, LabelSmoothingCrossEntropy and
SoftTargetCrossEntropy (loss/basic_loss.py:15-228) on the CPU, and weighted_hierarchical_loss (loss/hierarchical_loss.py:24-406) with
one task per criterion.

Runs only where the reference is mounted (see make_golden_hier_loss_soft.py, whose import recipe this follows):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen/make_golden_basic_loss.py

Per C in {2, 3, 257}, B = 16: logits, [B] targets (int64, with rows of class 0 and rows of other classes), [B, C] targets (convex
mixes of two classes with a tie-free maximum), a class weight [C] and an upstream gradient [B].  Recorded per criterion, per target
kind ("hard" / "rows"), with and without the weight, with and without ignore_index = 0, and for smoothing in {0, 0.1}: the per-sample
losses and the gradient of sum(go * loss) with respect to the logits.  The SoftTargetCrossEntropy rows are the [B, C] targets with row 5
scaled so that its entries sum to 0.8.  Key: <ce|ls|st>_C<C>_<hard|rows>_w<0|1>_i<0|1>[_s<0|1>]_<loss|grad>.

Then weighted_hierarchical_loss over three tasks (taxa_L10: CrossEntropyLoss, C = 257, [B] targets; taxa_L20:
LabelSmoothingCrossEntropy(0.1), C = 3, [B, C] targets; taxa_L30: SoftTargetCrossEntropy, C = 2, [B, C] targets), each criterion with
its class weight, in the four deterministic masking modes of hier_loss_soft.npz; in the phase1 mode the first two criteria carry
ignore_index = 0, as the reference's prepare_loss_functions builds them there.  Nothing from the reference is copied: the fixture holds
numbers only.
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
from linnaeus.loss.basic_loss import CrossEntropyLoss, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy  # noqa: E402
from linnaeus.loss.gradient_weighting import GradientWeighting  # noqa: E402
from linnaeus.loss.hierarchical_loss import weighted_hierarchical_loss  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SEED = 20251019
B = 16
CLASSES = (2, 3, 257)
MODES = (("sched1", 1.0, False, False), ("sched0", 0.0, False, False), ("phase1", 1.0, True, False), ("val", 0.0, False, True))
HIER = (("taxa_L10", 257, "ce"), ("taxa_L20", 3, "ls"), ("taxa_L30", 2, "st"))


class Sched:  # the one method the loss path calls (ops_schedule/ops_schedule.py:655)
    def __init__(self, p):
        self.p = p

    def get_null_mask_prob(self, step):
        return self.p


def run(crit, x, y, go):
    leaf = x.clone().requires_grad_(True)
    loss = crit(leaf, y)
    assert loss.shape == (B,)
    (loss * go).sum().backward()
    return loss.detach().numpy().copy(), leaf.grad.numpy().copy()


def main():
    g = torch.Generator().manual_seed(SEED)
    rec = {"classes": np.array(CLASSES)}
    data = {}
    for c in CLASSES:
        x = torch.randn(B, c, generator=g) * 2
        y = torch.randint(1, c, (B,), generator=g)
        y[[0, 3, 7, 12]] = 0  # the ignored rows under ignore_index = 0; null rows of the hierarchical loss
        a = torch.randint(1, c, (B,), generator=g)
        b = torch.randint(1, c, (B,), generator=g)
        a[:4] = 0   # rows 0..3: class 0 holds lam = 0.7 on even rows (null, and ignored after the arg-max), 0.35 on odd ones
        b[4:7] = 0  # rows 4..6: class 0 holds 1 - lam
        if c == 2:  # two classes: the other class is the other one
            b = 1 - a
        else:
            b = torch.where(a == b, (b % (c - 1)) + 1, b)
            b = torch.where(a == b, torch.zeros_like(b), b)
        lam = torch.where(torch.arange(B) % 2 == 0, torch.tensor(0.7), torch.tensor(0.35))
        rows = torch.zeros(B, c)
        rows[torch.arange(B), a] += lam
        rows[torch.arange(B), b] += 1.0 - lam
        assert (a != b).all() and ((rows == rows.max(1, keepdim=True).values).sum(1) == 1).all(), "a target row has a tied maximum"
        cls = rows.argmax(1)
        n_null = int((rows[:, 0] > 0.5).sum())
        assert 0 < n_null < B, n_null
        assert 0 < int((y == 0).sum()) < B and 0 < int((cls == 0).sum()) < B, "needs at least one ignored and one kept row"
        st_rows = rows.clone()
        st_rows[5] *= 0.8  # a row whose entries sum to 0.8: sum S is summed, not assumed
        assert abs(float(st_rows[5].sum()) - 0.8) < 1e-6 and int((st_rows > 0).sum(1).min()) == 2
        w = 0.5 + torch.rand(c, generator=g)
        go = 0.5 + torch.rand(B, generator=g)
        data[c] = (x, y, rows, st_rows, w)
        rec[f"logits_C{c}"], rec[f"hard_C{c}"], rec[f"rows_C{c}"], rec[f"strows_C{c}"] = x.numpy(), y.numpy(), rows.numpy(), st_rows.numpy()
        rec[f"weight_C{c}"], rec[f"go_C{c}"] = w.numpy(), go.numpy()
        for kind, tgt in (("hard", y), ("rows", rows)):
            for wi in (0, 1):
                for ii in (0, 1):
                    kw = dict(weight=w if wi else None, apply_class_weights=bool(wi), ignore_index=0 if ii else None)
                    key = f"ce_C{c}_{kind}_w{wi}_i{ii}"
                    rec[key + "_loss"], rec[key + "_grad"] = run(CrossEntropyLoss(**kw), x, tgt, go)
                    if ii:
                        zero = (tgt if kind == "hard" else cls) == 0
                        assert (rec[key + "_loss"][zero.numpy()] == 0).all() and (rec[key + "_grad"][zero.numpy()] == 0).all()
                    for si, eps in enumerate((0.0, 0.1)):
                        key = f"ls_C{c}_{kind}_w{wi}_i{ii}_s{si}"
                        rec[key + "_loss"], rec[key + "_grad"] = run(LabelSmoothingCrossEntropy(smoothing=eps, **kw), x, tgt, go)
        for wi in (0, 1):
            key = f"st_C{c}_rows_w{wi}_i0"
            rec[key + "_loss"], rec[key + "_grad"] = run(SoftTargetCrossEntropy(weight=w if wi else None, apply_class_weights=bool(wi)), x, st_rows, go)
        print(f"[basic_loss] C={c}: {int((y == 0).sum())} rows of class 0, {n_null} null rows among the [B, C] targets")

    tasks = [t for t, _, _ in HIER]
    tw = {t: float(0.3 + torch.rand(1, generator=g).item()) for t in tasks}
    rec["tasks"], rec["task_weights"] = np.array(tasks), np.array([tw[t] for t in tasks])
    rec["hier_classes"], rec["hier_kinds"] = np.array([c for _, c, _ in HIER]), np.array([k for _, _, k in HIER])
    logits, targets, cw = {}, {}, {}
    for t, c, kind in HIER:
        x, y, rows, st_rows, w = data[c]
        logits[t] = x.clone().requires_grad_(True)
        targets[t] = {"ce": y, "ls": rows, "st": st_rows}[kind]
        cwv = 0.5 + torch.rand(c, generator=g)
        cw[t] = {i: float(cwv[i]) for i in range(0, c, 2)}  # a sparse dict, as hier_loss.npz: missing -> 1.0
        rec[f"cw_{t}"] = cwv.numpy()
    for mode, prob, phase1, val in MODES:
        cfg = get_default_config()
        cfg.defrost()
        cfg.TRAIN.PHASE1_MASK_NULL_LOSS = phase1
        ign = 0 if phase1 else None
        criteria = {}
        for t, c, kind in HIER:
            w = data[c][4]
            criteria[t] = {"ce": lambda: CrossEntropyLoss(weight=w, apply_class_weights=True, ignore_index=ign),
                           "ls": lambda: LabelSmoothingCrossEntropy(weight=w, smoothing=0.1, apply_class_weights=True, ignore_index=ign),
                           "st": lambda: SoftTargetCrossEntropy(weight=w, apply_class_weights=True)}[kind]()
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
        print(f"[basic_loss/{mode}] total {total.item():.6f} weighted {rec[f'{mode}_weighted']}")
    path = os.path.join(OUT, "basic_loss.npz")
    np.savez_compressed(path, **rec)
    print(f"[basic_loss] {len(rec)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
