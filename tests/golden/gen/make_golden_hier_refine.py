#!/usr/bin/env python3
"""Generate tests/golden/hier_refine.npz from the reference's own hierarchical heads (linnaeus/models/heads/hierarchical_softmax_head.py,
conditional_classifier_head.py), unmodified, on its own TaxonomyTree (linnaeus/utils/taxonomy/taxonomy_tree.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_hier_refine.py <linnaeus checkout>

In a model the reference's refinement never runs (the tree names its matrices "{parent}_{child}", the heads look up
"{task_keys[i]}_{task_keys[i+1]}" with task_keys finest first).  Constructed with task_keys = reversed(tree.task_keys) the same
HierarchicalSoftmaxHead.forward finds every matrix and computes base + log(softmax(parent) . M + 1e-10) from the coarsest rank down:
that is what is recorded here.  ConditionalClassifierHead.forward raises even then (F4), but its _compute_routing_probabilities is
callable on its own.  Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/, runs on CPU in fp32.
Writes numbers only:

  tree      four ranks taxa_L10 .. taxa_L40 with (11, 6, 4, 2) classes and uneven fan-out: parents with 1 .. 4 children, taxa_L20
            class 5 and taxa_L30 class 3 without children, class 0 of the three finer ranks without a parent; `parent_<task>` =
            the hierarchy map as an array (-1 = none), `hmatrix_<parent>_<child>` = the tree's own matrix
  inputs    `x` [5, 16] seeded fp32 features, `weight_<task>` / `bias_<task>` of the shared per-level classifiers
  hsm       `base_<task>` (the classifiers' outputs, from forward hooks), `out_<task>` = the head's output with that primary task,
            `probe_<task>` = seeded weights of the probe loss sum_t (out_t * probe_t).sum(), `dbase_<task>` = its gradient with
            respect to the level's base logits (retain_grad on every classifier output, summed over the calls of the four heads)
  routing   `route_logits` [5, 6]; `route_soft` (routing 'soft', temperature 0.7), `route_hard` ('hard', eval), `route_gumbel`
            ('gumbel', training, temperature 0.5, torch.manual_seed(GUMBEL_SEED)) and `gumbel_noise`, regenerated from that seed as
            F.gumbel_softmax draws it and asserted to reproduce `route_gumbel`
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "models", "heads", "hierarchical_softmax_head.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(HERE, "_stubs"), REF]
sys.dont_write_bytecode = True

import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

warnings.filterwarnings("ignore")
logging.disable(logging.CRITICAL)

from linnaeus.models.heads.conditional_classifier_head import ConditionalClassifierHead  # noqa: E402
from linnaeus.models.heads.hierarchical_softmax_head import HierarchicalSoftmaxHead  # noqa: E402
from linnaeus.utils.taxonomy.taxonomy_tree import TaxonomyTree  # noqa: E402

SEED = 20250611
GUMBEL_SEED = 4242
KEYS = ["taxa_L10", "taxa_L20", "taxa_L30", "taxa_L40"]  # finest first
CLASSES = {"taxa_L10": 11, "taxa_L20": 6, "taxa_L30": 4, "taxa_L40": 2}
HIERARCHY = {  # child task -> {child class: parent class in the next task}; class 0 has no entry
    "taxa_L10": {1: 1, 2: 1, 3: 1, 4: 1, 5: 2, 6: 3, 7: 3, 8: 4, 9: 4, 10: 4},  # taxa_L20 class 5: no children
    "taxa_L20": {1: 0, 2: 1, 3: 1, 4: 2, 5: 2},                                 # taxa_L30 class 3: no children
    "taxa_L30": {1: 0, 2: 1, 3: 1},
}
B, FEATS = 5, 16
SOFT_T, GUMBEL_T = 0.7, 0.5


def main():
    tree = TaxonomyTree(HIERARCHY, KEYS, CLASSES)
    mats = tree.build_hierarchy_matrices()
    rec = {"task_keys": np.array(KEYS), "num_classes": np.array([CLASSES[k] for k in KEYS])}
    for i in range(len(KEYS) - 1):
        child, parent = KEYS[i], KEYS[i + 1]
        m = mats[f"{parent}_{child}"]
        assert tuple(m.shape) == (CLASSES[parent], CLASSES[child])
        par = np.array([HIERARCHY[child].get(c, -1) for c in range(CLASSES[child])], dtype=np.int32)
        for c in range(CLASSES[child]):  # the array, the tree's get_parent and the tree's matrix say the same
            node = tree.get_parent((child, c))
            assert (node[1] if node is not None else -1) == par[c]
            assert m[:, c].sum().item() == (1.0 if par[c] >= 0 else 0.0) and (par[c] < 0 or m[par[c], c].item() == 1.0)
        rec[f"parent_{child}"] = par
        rec[f"hmatrix_{parent}_{child}"] = m.numpy().astype(np.float32)

    g = torch.Generator().manual_seed(SEED)
    shared = nn.ModuleDict({k: nn.Linear(FEATS, CLASSES[k]) for k in KEYS})
    for k in KEYS:
        with torch.no_grad():
            shared[k].weight.copy_(torch.randn(CLASSES[k], FEATS, generator=g) * 0.6)
            shared[k].bias.copy_(torch.randn(CLASSES[k], generator=g) * 0.3)
        rec[f"weight_{k}"], rec[f"bias_{k}"] = shared[k].weight.detach().numpy().copy(), shared[k].bias.detach().numpy().copy()
    x = torch.randn(B, FEATS, generator=g)
    rec["x"] = x.numpy()
    probe = {k: torch.randn(B, CLASSES[k], generator=g) for k in KEYS}

    order = list(reversed(tree.task_keys))  # coarsest first: now the heads' pair keys are the tree's
    assert order == list(reversed(KEYS))
    seen = {k: [] for k in KEYS}
    hooks = []
    for k in KEYS:
        def keep(mod, inp, out, k=k):
            out.retain_grad()
            seen[k].append(out)
        hooks.append(shared[k].register_forward_hook(keep))
    heads = {k: HierarchicalSoftmaxHead(FEATS, k, order, tree, CLASSES, level_classifiers_override=shared) for k in KEYS}
    outs = {k: heads[k](x) for k in KEYS}
    loss = sum((outs[k] * probe[k]).sum() for k in KEYS)
    loss.backward()
    for h in hooks:
        h.remove()
    for k in KEYS:
        assert len(seen[k]) == len(KEYS) and all(torch.equal(t, seen[k][0]) for t in seen[k])
        rec[f"base_{k}"] = seen[k][0].detach().numpy().copy()
        rec[f"out_{k}"] = outs[k].detach().numpy().copy()
        rec[f"probe_{k}"] = probe[k].numpy().copy()
        rec[f"dbase_{k}"] = sum(t.grad for t in seen[k] if t.grad is not None).numpy().copy()
    # the refinement did fire: every finer rank differs from its base, the coarsest does not
    assert all(not np.allclose(rec[f"out_{k}"], rec[f"base_{k}"]) for k in KEYS[:-1]) and np.array_equal(rec[f"out_{KEYS[-1]}"], rec[f"base_{KEYS[-1]}"])
    # and it is the formula, chained from the coarsest rank
    ref = {KEYS[-1]: seen[KEYS[-1]][0].detach().double()}
    for i in range(len(KEYS) - 2, -1, -1):
        child, parent = KEYS[i], KEYS[i + 1]
        ref[child] = seen[child][0].detach().double() + torch.log(torch.softmax(ref[parent], 1) @ mats[f"{parent}_{child}"].double() + 1e-10)
        assert torch.allclose(outs[child].detach().double(), ref[child], rtol=1e-5, atol=1e-5)

    logits = torch.randn(B, CLASSES["taxa_L20"], generator=g) * 2.0
    logits[1, 2] = logits[1, 4] = logits[1].max() + 1.0  # a tie for the arg-max: torch.argmax takes the lower index
    rec["route_logits"] = logits.numpy().copy()
    rec["soft_temperature"], rec["gumbel_temperature"] = np.float32(SOFT_T), np.float32(GUMBEL_T)

    def cch(strategy, temperature, training):
        h = ConditionalClassifierHead(FEATS, "taxa_L10", order, tree, CLASSES, routing_strategy=strategy, temperature=temperature,
                                      level_classifiers_override=shared)
        h.train(training)
        return h

    with torch.no_grad():
        rec["route_soft"] = cch("soft", SOFT_T, True)._compute_routing_probabilities(logits).numpy().copy()
        rec["route_hard"] = cch("hard", 1.0, False)._compute_routing_probabilities(logits).numpy().copy()
        assert rec["route_hard"][1].argmax() == 2 and rec["route_hard"].sum() == B
        torch.manual_seed(GUMBEL_SEED)
        rec["route_gumbel"] = cch("gumbel", GUMBEL_T, True)._compute_routing_probabilities(logits).numpy().copy()
        torch.manual_seed(GUMBEL_SEED)
        noise = -torch.empty_like(logits).exponential_().log()
        again = torch.softmax((logits + noise) / GUMBEL_T, dim=1)
        assert torch.equal(again, torch.from_numpy(rec["route_gumbel"])), "regenerated gumbel noise does not reproduce the reference's probabilities"
        rec["gumbel_noise"] = noise.numpy().copy()
        # hard in training and gumbel in eval fall back to soft routing
        assert torch.equal(cch("hard", SOFT_T, True)._compute_routing_probabilities(logits), torch.from_numpy(rec["route_soft"]))
        assert torch.equal(cch("gumbel", SOFT_T, False)._compute_routing_probabilities(logits), torch.from_numpy(rec["route_soft"]))

    path = os.path.join(REPO, "tests", "golden", "hier_refine.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes;", len(rec), "arrays")


if __name__ == "__main__":
    main()
