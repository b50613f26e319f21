#!/usr/bin/env python3
"""Generate tests/golden/gradnorm.npz and tests/golden/gradnorm_backbone_sm.json from the reference's own GradNorm
(linnaeus/loss/gradient_weighting.py update_gradnorm_weights_reforward, linnaeus/loss/gradnorm.py GradNormModule).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_gradnorm.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/ and runs on CPU in fp32.  Writes
numbers and names only:

  e2e cases (tiny_a of tests/cases.py, batch 4 at 64 px, seeded weights of oracle.mformer_oracle, drop rates 0, two
  successive updates on two seeded batches with some null targets, TaxonomyAwareLabelSmoothingCE criteria):
    c0  ALPHA 1.5, ZERO_AUX_INFO on,  GRADNORM_ACCUM_STEPS 1, ENABLED_GRADNORM_STEPS on  (recompute plan)
    c1  ALPHA 0,   ZERO_AUX_INFO off, GRADNORM_ACCUM_STEPS 2, ENABLED_GRADNORM_STEPS off
    c2  ALPHA 1.5, ZERO_AUX_INFO off, GRADNORM_ACCUM_STEPS 2, ENABLED_GRADNORM_STEPS on
  Per call: the metrics (sorted-key order), the task_weights / initial_losses buffers after the call, and which
  parameters' .grad are None afterwards (every .grad is populated by a probe backward before each call).
  Before each call: the targets of the batch (the images and metadata are oracle.mformer_oracle.seeded_inputs).

  measure_and_update known answers (k0..k2) on synthetic losses and flat gradients: unsorted task keys, alpha 1.5 with a
  second call, alpha 0, and a task whose target is below 1e-8.

  gradnorm_backbone_sm.json: the parameter names GradientWeighting.set_model selects as the backbone of the reference-built
  mFormerV1_sm (default EXCLUDE_CONFIG), in named_parameters order.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "loss", "gradnorm.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(HERE, "_stubs"), REPO, REF, HERE]
sys.dont_write_bytecode = True

import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

warnings.filterwarnings("ignore")
logging.disable(logging.CRITICAL)

from oracle import mformer_oracle as O  # noqa: E402
from tests.cases import CASES, SEED  # noqa: E402

import make_golden as MG  # noqa: E402  (after tests.cases: it puts the checkout, whose tests/ package differs, first on the path)
from linnaeus.loss.gradient_weighting import GradientWeighting  # noqa: E402
from linnaeus.loss.gradnorm import GradNormModule  # noqa: E402
from linnaeus.loss.taxonomy_label_smoothing import TaxonomyAwareLabelSmoothingCE  # noqa: E402
from linnaeus.models import build_model  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
CASES_E2E = {
    "c0": dict(alpha=1.5, zero_aux=True, accum=1, ckpt=True),
    "c1": dict(alpha=0.0, zero_aux=False, accum=2, ckpt=False),
    "c2": dict(alpha=1.5, zero_aux=False, accum=2, ckpt=True),
}
BATCH, IMG = 4, 64


def soft_matrix(c, a):
    m = torch.full((c, c), a / (c - 1))
    m.fill_diagonal_(1.0 - a)
    return m


def batch_for(spec, call):
    x, meta = O.seeded_inputs(spec, BATCH, IMG, SEED + 100 + call)
    g = torch.Generator().manual_seed(SEED + 200 + call)
    targets = {}
    for t, c in spec.heads:
        y = torch.randint(1, c, (BATCH,), generator=g)
        y[torch.rand(BATCH, generator=g) < 0.35] = 0  # null labels
        targets[t] = y
    targets[spec.heads[0][0]][0] = 0  # at least one null row
    return x, meta, targets


def run_e2e(rec):
    spec = CASES["tiny_a"]
    tasks = [t for t, _ in spec.heads]
    for t, c in spec.heads:
        rec[f"soft_{t}"] = soft_matrix(c, 0.1).numpy()
    for name, cc in CASES_E2E.items():
        cfg = MG.apply_spec(MG.base_cfg(IMG), spec)
        cfg.MODEL.DROP_RATE = 0.0
        cfg.MODEL.DROP_PATH_RATE = 0.0
        T = cfg.LOSS.GRAD_WEIGHTING.TASK
        T.ALPHA = cc["alpha"]
        T.ZERO_AUX_INFO = cc["zero_aux"]
        T.GRADNORM_ACCUM_STEPS = cc["accum"]
        cfg.TRAIN.GRADIENT_CHECKPOINTING.ENABLED_GRADNORM_STEPS = cc["ckpt"]
        model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
        MG.load_seeded(model, SEED)
        model.train()
        criteria = {t: TaxonomyAwareLabelSmoothingCE(soft_matrix(c, 0.1)) for t, c in spec.heads}
        gw = GradientWeighting(tasks, cfg, "gradnorm", alpha=cc["alpha"], zero_aux_info=cc["zero_aux"])
        gw.set_model(model)
        names = [n for n, _ in model.named_parameters()]
        rec[f"{name}_backbone"] = np.array([any(p is q for q in gw.backbone_params) for _, p in model.named_parameters()])
        for call in range(2):
            x, meta, targets = batch_for(spec, call)
            if name == "c0":  # (the same batches in every case; the images are O.seeded_inputs(spec, BATCH, IMG, SEED + 100 + call))
                rec[f"x_sum_{call}"] = np.array(float(x.double().sum()))
            for t in tasks:
                rec[f"target_{call}_{t}"] = targets[t].numpy()
            model.zero_grad(set_to_none=True)
            O.probe_loss(model(x, meta)).backward()
            metrics = gw.update_gradnorm_weights_reforward((x, targets, meta), criteria, amp_enabled=False, current_step=call)
            keys = sorted(metrics.keys())
            rec[f"{name}_{call}_metric_keys"] = np.array(keys)
            rec[f"{name}_{call}_metrics"] = np.array([metrics[k] for k in keys], dtype=np.float64)
            rec[f"{name}_{call}_weights"] = gw.gradnorm.task_weights.numpy().copy()
            rec[f"{name}_{call}_initial_losses"] = gw.gradnorm.initial_losses.numpy().copy()
            rec[f"{name}_{call}_grad_none"] = np.array([p.grad is None for _, p in model.named_parameters()])
        rec[f"{name}_param_names"] = np.array(names)


def run_known_answers(rec):
    g = torch.Generator().manual_seed(SEED + 300)
    cases = {
        # unsorted keys; alpha 1.5, two calls (the second reuses initial_losses)
        "k0": dict(keys=["taxa_L30", "taxa_L10", "taxa_L20"], alpha=1.5, init=[1.0, 2.0, 0.5], scale=[1.0, 3.0, 0.2]),
        # alpha 0: equalise the norms
        "k1": dict(keys=["taxa_L20", "taxa_L10"], alpha=0.0, init=[1.0, 1.0], scale=[2.0, 0.5]),
        # a task whose target is below 1e-8 (zero loss ratio) keeps its weight before the renormalisation
        "k2": dict(keys=["taxa_L10", "taxa_L40", "taxa_L20", "taxa_L30"], alpha=1.5, init=[1.0, 1.0, 1.0, 1.0], scale=[1.0, 1.0, 1.0, 1.0], zero="taxa_L40"),
    }
    for name, cc in cases.items():
        keys = cc["keys"]
        mod = GradNormModule(keys, alpha=cc["alpha"], init_weights=torch.tensor(cc["init"]))
        rec[f"{name}_keys"] = np.array(keys)
        rec[f"{name}_alpha"] = np.array(cc["alpha"])
        rec[f"{name}_init"] = np.array(cc["init"], dtype=np.float32)
        for call in range(2):
            losses = {k: torch.rand((), generator=g) * 2 + 0.1 for k in keys}
            grads = {k: torch.randn(257, generator=g) * s for k, s in zip(keys, cc["scale"])}
            if cc.get("zero") and call == 1:
                losses[cc["zero"]] = torch.zeros(())
            metrics = mod.measure_and_update(losses, grads)
            rec[f"{name}_{call}_loss"] = np.array([float(losses[k]) for k in keys], dtype=np.float32)
            rec[f"{name}_{call}_norm"] = np.array([float(grads[k].norm()) for k in keys], dtype=np.float32)
            mk = sorted(metrics.keys())
            rec[f"{name}_{call}_metric_keys"] = np.array(mk)
            rec[f"{name}_{call}_metrics"] = np.array([metrics[k] for k in mk], dtype=np.float64)
            rec[f"{name}_{call}_weights"] = mod.task_weights.numpy().copy()
            rec[f"{name}_{call}_initial_losses"] = mod.initial_losses.numpy().copy()


def backbone_names_sm():
    spec = CASES["sm"]
    cfg = MG.apply_spec(MG.base_cfg(224), spec)
    model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    gw = GradientWeighting([t for t, _ in spec.heads], cfg, "gradnorm")
    gw.set_model(model)
    ids = {id(p) for p in gw.backbone_params}
    return [n for n, p in model.named_parameters() if id(p) in ids]


def main():
    torch.manual_seed(SEED)
    rec = {}
    run_e2e(rec)
    run_known_answers(rec)
    np.savez_compressed(os.path.join(OUT, "gradnorm.npz"), **rec)
    with open(os.path.join(OUT, "gradnorm_backbone_sm.json"), "w") as f:
        json.dump(backbone_names_sm(), f, indent=0)
        f.write("\n")
    print("wrote", os.path.join(OUT, "gradnorm.npz"), os.path.getsize(os.path.join(OUT, "gradnorm.npz")), "bytes")


if __name__ == "__main__":
    main()
