#!/usr/bin/env python3
"""Generate tests/golden/optim_build.json and tests/golden/optim_step.npz from the reference's own optimizer builder
(linnaeus/optimizers/build.py, multi_optimizer.py, muon.py) and the clip block of its training loop (train.py:279-313).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_optim_build.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/, runs on the CPU and writes names and
numbers only.

optim_build.json: `build_optimizer(config, model)` on the reference-built mFormerV1_sm with the four heads of tests/cases.py, for
  sgd, adamw, ademamix, muon    OPTIMIZER.NAME, no parameter groups
  pg_muon    parameter groups: HEADS (name filter "head", adamw, LR_MULTIPLIER 10, WEIGHT_DECAY 0), ROPE (name startswith
             "stages.2", muon, LR_MULTIPLIER 0.5: its 1-D parameters give ROPE_ADAMW), DEFAULT = muon
  pg_sgd     parameter groups: VECTORS (dimension 1, ademamix, WEIGHT_DECAY 0), DEFAULT = sgd with WEIGHT_DECAY 0.01
{"names": named_parameters() order, "dims": their dim(), "configs": {config: {"overrides": the OPTIMIZER node that was set,
"kind": MultiOptimizer or the optimizer's class, "optimizers": {name: {"class", "ordered": whether the parameter order is the
reference's own (False where it iterates a Python set), "groups": [{"params": indices into names, hyper-parameters...}]}}}}}.
The flattened wrappers Muon is given for 4-D weights are mapped back to the weight's name by data_ptr().

optim_step.npz: three steps of train.py:279-313 -- clip_grad_norm_(all, inf), clip_grad_norm_(all, c), the post-clip norm measured
again, MultiOptimizer.step -- with {"MUON": Muon([48x192, 40x100]), "ADAMW": AdamW([4097, 33x7]), "SGD": SGD([1025, 5], momentum
0.9, nesterov, weight_decay 0.05)}, bf16-exact initial values and gradients, c = CLIP chosen so that step 0 clips and step 2 does
not.  Recorded: initial values, gradients as given, parameters after every step, the three norms per step, the final AdamW / SGD
states and Muon buffers.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "optimizers", "build.py")):
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

from tests.cases import CASES  # noqa: E402

import make_golden as MG  # noqa: E402  (after tests.cases: it puts the checkout, whose tests/ package differs, first on the path)
from linnaeus.models import build_model  # noqa: E402
from linnaeus.optimizers.build import build_optimizer  # noqa: E402
from linnaeus.optimizers.multi_optimizer import MultiOptimizer  # noqa: E402
from linnaeus.optimizers.muon import Muon  # noqa: E402
from yacs.config import CfgNode as CN  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SEED = 20261020

PG_MUON = {"ENABLED": True,
           "DEFAULT": {"OPTIMIZER": "muon", "WEIGHT_DECAY": 0.05, "LR_MULTIPLIER": 1.0},
           "HEADS": {"FILTER": {"TYPE": "name", "PATTERNS": ["head"]}, "OPTIMIZER": "adamw", "LR_MULTIPLIER": 10.0, "WEIGHT_DECAY": 0.0},
           "ROPE": {"FILTER": {"TYPE": "name", "PATTERNS": ["stages.2"], "MATCH_TYPE": "startswith"}, "OPTIMIZER": "muon", "LR_MULTIPLIER": 0.5}}
PG_SGD = {"ENABLED": True,
          "DEFAULT": {"OPTIMIZER": "sgd", "WEIGHT_DECAY": 0.01, "LR_MULTIPLIER": 1.0},
          "VECTORS": {"FILTER": {"TYPE": "dimension", "DIMENSIONS": [1]}, "OPTIMIZER": "ademamix", "WEIGHT_DECAY": 0.0}}
CONFIGS = {
    "sgd": {"NAME": "sgd"}, "adamw": {"NAME": "adamw"}, "ademamix": {"NAME": "ademamix", "T_ALPHA_BETA3": 1000.0}, "muon": {"NAME": "muon"},
    "pg_muon": {"NAME": "adamw", "PARAMETER_GROUPS": PG_MUON}, "pg_sgd": {"NAME": "adamw", "PARAMETER_GROUPS": PG_SGD},
}


def jsonable(v):
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if isinstance(v, (tuple, list)) and all(isinstance(x, (bool, int, float)) for x in v):
        return list(v)
    return None


def describe(opt, index_of, ordered):
    groups = []
    for g in opt.param_groups:
        d = {"params": [index_of[p.data_ptr()] for p in g["params"]]}
        for k, v in g.items():
            if k != "params" and (jsonable(v) is not None or v is None):
                d[k] = jsonable(v)
        groups.append(d)
    return {"class": type(opt).__name__, "ordered": ordered, "groups": groups}


def build_cases():
    spec = CASES["sm"]
    out = {"configs": {}}
    for cname, over in CONFIGS.items():
        cfg = MG.apply_spec(MG.base_cfg(224), spec)
        cfg.defrost()
        for k, v in over.items():
            cfg.OPTIMIZER[k] = CN(v) if isinstance(v, dict) else v
        torch.manual_seed(SEED)
        model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
        named = list(model.named_parameters())
        if "names" not in out:
            out["names"] = [n for n, _ in named]
            out["dims"] = [p.dim() for _, p in named]
        assert out["names"] == [n for n, _ in named]
        index_of = {p.data_ptr(): i for i, (_, p) in enumerate(named)}
        assert len(index_of) == len(named)
        opt = build_optimizer(cfg, model)
        rec = {"overrides": over, "base_lr": float(cfg.LR_SCHEDULER.BASE_LR), "clip_grad": float(cfg.TRAIN.CLIP_GRAD)}
        if isinstance(opt, MultiOptimizer):
            rec["kind"] = "MultiOptimizer"
            # the DEFAULT* optimizers of the parameter-group path take their parameters from a Python set: no order to compare
            rec["optimizers"] = {n: describe(o, index_of, not (cname.startswith("pg_") and n.startswith("DEFAULT"))) for n, o in opt.optimizers.items()}
            rec["param_group_tags"] = [[g["optimizer_name"], g["optimizer_group_idx"]] for g in opt.param_groups]
        else:
            rec["kind"] = type(opt).__name__
            rec["optimizers"] = {"": describe(opt, index_of, True)}
        out["configs"][cname] = rec
    return out


# ------------------------------------------------------------------------------------------------------------------ three steps
SHAPES = {"MUON": [(48, 192), (40, 100)], "ADAMW": [(4097,), (33, 7)], "SGD": [(1025,), (5,)]}
HYPER = {"MUON": dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5),
         "ADAMW": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05),
         "SGD": dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=0.05)}
GRAD_SCALE = [1.0, 0.3, 0.05]  # per step: the norm falls through the clip value
CLIP = 20.0
STEPS = 3


def bf16_exact(t):
    return t.to(torch.bfloat16).float()


def run_steps():
    gen = torch.Generator().manual_seed(SEED)
    params = {k: [torch.nn.Parameter(bf16_exact(torch.randn(*s, generator=gen) * 0.1)) for s in v] for k, v in SHAPES.items()}
    rec = {"clip": np.array(CLIP), "steps": np.array(STEPS)}
    for k, ps in params.items():
        for i, p in enumerate(ps):
            rec[f"{k}_{i}_init"] = p.detach().numpy().copy()
    opts = {"MUON": Muon(params["MUON"], **HYPER["MUON"]), "ADAMW": torch.optim.AdamW(params["ADAMW"], **HYPER["ADAMW"]),
            "SGD": torch.optim.SGD(params["SGD"], **HYPER["SGD"])}
    multi = MultiOptimizer(opts)
    every = [p for ps in params.values() for p in ps]
    norms = np.zeros((STEPS, 3), dtype=np.float64)
    for s in range(STEPS):
        for k, ps in params.items():
            for i, p in enumerate(ps):
                g = bf16_exact(torch.randn(p.shape, generator=gen) * GRAD_SCALE[s])
                rec[f"{k}_{i}_grad{s}"] = g.numpy().copy()
                p.grad = g.clone()
        # train.py:282-308
        to_clip = [p for p in every if p.grad is not None]
        norms[s, 0] = torch.nn.utils.clip_grad_norm_(to_clip, float("inf")).item()
        norms[s, 2] = torch.nn.utils.clip_grad_norm_(to_clip, CLIP).item()
        norms[s, 1] = torch.linalg.norm(torch.cat([p.grad.detach().flatten() for p in to_clip]).float()).item()
        multi.step()
        for k, ps in params.items():
            for i, p in enumerate(ps):
                rec[f"{k}_{i}_after{s}"] = p.detach().numpy().copy()
    assert norms[0, 0] > CLIP > norms[2, 0], norms
    rec["norms"] = norms
    for i, p in enumerate(params["MUON"]):
        rec[f"MUON_{i}_buf"] = opts["MUON"].state[p]["momentum_buffer"].numpy().copy()
    for i, p in enumerate(params["ADAMW"]):
        st = opts["ADAMW"].state[p]
        rec[f"ADAMW_{i}_exp_avg"], rec[f"ADAMW_{i}_exp_avg_sq"] = st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()
        rec[f"ADAMW_{i}_step"] = np.array(float(st["step"]))
    for i, p in enumerate(params["SGD"]):
        rec[f"SGD_{i}_buf"] = opts["SGD"].state[p]["momentum_buffer"].numpy().copy()
    # finding: MultiOptimizer.state_dict() saves no optimizer state
    rec["ref_state_dict_state_sizes"] = np.array([len(v["state"]) for v in multi.state_dict()["optimizers"].values()])
    return rec


def main():
    built = build_cases()
    with open(os.path.join(OUT, "optim_build.json"), "w") as f:
        json.dump(built, f, separators=(",", ":"))
        f.write("\n")
    print("wrote optim_build.json", os.path.getsize(os.path.join(OUT, "optim_build.json")), "bytes")
    with torch.backends.mkldnn.flags(enabled=False):  # as make_golden_muon_fused.py: the same bf16 matmul bits on every CPU
        rec = run_steps()
    np.savez_compressed(os.path.join(OUT, "optim_step.npz"), **rec)
    print("wrote optim_step.npz", os.path.getsize(os.path.join(OUT, "optim_step.npz")), "bytes;  norms", rec["norms"].tolist())


if __name__ == "__main__":
    main()
