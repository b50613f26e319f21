#!/usr/bin/env python3
"""Generate tests/golden/taxonomy_tables.npz from the *reference itself*: TaxonomyTree.build_distance_matrix
(utils/taxonomy/taxonomy_tree.py:364-381), build_taxonomy_smoothing_matrix and TaxonomyAwareLabelSmoothingCE
(loss/taxonomy_label_smoothing.py:30-128, 131-408) and generate_taxonomy_matrices (utils/taxonomy/taxonomy_utils.py:24-254).

Runs only where the reference is mounted (see make_golden.py, whose import recipe this follows):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/gen/make_golden_taxonomy_tables.py

Four seeded forests of four levels (tests/taxonomy_ref.py: random_forest -- parentless classes, chains broken one level up, a
single-child parent, a top level of global roots), leaf C <= 96.  Per forest f: the parent arrays `f{f}_parents_{l}`; per level l
the distances `f{f}_l{l}_dist`; per setting s of taxonomy_ref.SETTINGS the matrix `f{f}_l{l}_s{s}_soft` and, on seeded logits
(B = 6, targets with class 0 under ignore_index = 0, a class weight), the criterion's `..._loss` and `..._grad`.  The last setting
(beta = 20) forces the near-zero-sum fallback: exp(-40) * C is far below 1e-9 in fp32 and in fp64.  For forest 0,
generate_taxonomy_matrices under two stub configs (`gen{g}_*`), the top level taking the uniform branch.  One forest with leaf
C = 257 (`big_*`): distances and the first setting only.  Nothing from the reference is copied: the fixture holds numbers only.
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
from linnaeus.loss.taxonomy_label_smoothing import TaxonomyAwareLabelSmoothingCE, build_taxonomy_smoothing_matrix  # noqa: E402
from linnaeus.utils.taxonomy.taxonomy_tree import TaxonomyTree  # noqa: E402
from linnaeus.utils.taxonomy.taxonomy_utils import generate_taxonomy_matrices  # noqa: E402

sys.path.insert(0, os.path.join(REPO, "tests"))  # (the reference has a `tests` package of its own)
from taxonomy_ref import SETTINGS, hierarchy_map, random_forest  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
SEED = 20261020
KEYS = ["taxa_L10", "taxa_L20", "taxa_L30", "taxa_L40"]
FORESTS = ([96, 24, 7, 3], [61, 17, 5, 2], [40, 12, 6, 4], [83, 9, 3, 2])
BIG = [257, 40, 9, 3]
B = 6
# (enabled flags, uniform_roots, fallback_to_uniform) of the generate_taxonomy_matrices cases
GEN = (([True, True, True, True], True, True), ([True, False, True, True], False, False))


def tree_of(parents, ncls):
    return TaxonomyTree(hierarchy_map(parents, KEYS), list(KEYS), dict(zip(KEYS, ncls)))


def roots_at(tree, key):
    return [i for i, nd in enumerate(tree.get_nodes_at_level(key)) if tree.get_parent(nd) is None]


def main():
    rng = np.random.default_rng(SEED)
    g = torch.Generator().manual_seed(SEED + 1)
    rec = {"keys": np.array(KEYS), "forests": np.array(FORESTS), "big": np.array(BIG), "settings": np.array(SETTINGS, np.float64)}
    for f, ncls in enumerate(FORESTS):
        parents = random_forest(rng, ncls)
        tree = tree_of(parents, ncls)
        for lv, key in enumerate(KEYS):
            rec[f"f{f}_parents_{lv}"] = parents[lv]
            Cn = ncls[lv]
            dist = tree.build_distance_matrix(key)
            rec[f"f{f}_l{lv}_dist"] = dist.numpy()
            logits = torch.randn(B, Cn, generator=g) * 2
            target = torch.randint(0, Cn, (B,), generator=g)
            target[0], target[1], target[2] = 0, 1, min(2, Cn - 1)  # the ignored class, a parentless class, a broken chain
            cw = torch.rand(Cn, generator=g) + 0.5
            rec[f"f{f}_l{lv}_logits"], rec[f"f{f}_l{lv}_target"], rec[f"f{f}_l{lv}_cw"] = logits.numpy(), target.numpy(), cw.numpy()
            for s, (alpha, beta, ur) in enumerate(SETTINGS):
                soft = build_taxonomy_smoothing_matrix(Cn, dist, alpha, beta, ur, roots_at(tree, key))
                rec[f"f{f}_l{lv}_s{s}_soft"] = soft.numpy()
                crit = TaxonomyAwareLabelSmoothingCE(soft, weight=cw, apply_class_weights=True, ignore_index=0)
                x = logits.clone().requires_grad_(True)
                loss = crit(x, target)
                loss.sum().backward()
                rec[f"f{f}_l{lv}_s{s}_loss"], rec[f"f{f}_l{lv}_s{s}_grad"] = loss.detach().numpy(), x.grad.numpy().copy()
        print(f"[taxonomy_tables] forest {f}: classes {ncls}, parentless per level {[int((p < 0).sum()) for p in parents]}")
        if f == 0:
            for gi, (flags, ur, fb) in enumerate(GEN):
                cfg = get_default_config()
                cfg.defrost()
                cfg.DATA.TASK_KEYS_H5 = list(KEYS)
                ts = cfg.LOSS.TAXONOMY_SMOOTHING
                ts.ENABLED, ts.ALPHA, ts.BETA, ts.UNIFORM_ROOTS, ts.FALLBACK_TO_UNIFORM = list(flags), 0.2, 0.5, ur, fb
                nc = dict(zip(KEYS, ncls))
                mats = generate_taxonomy_matrices(cfg, tree, nc)
                rec[f"gen{gi}_tasks"] = np.array(sorted(mats))
                rec[f"gen{gi}_cfg"] = np.array([0.2, 0.5, float(ur), float(fb)] + [float(x) for x in flags])
                for t, m in mats.items():
                    rec[f"gen{gi}_{t}"] = m.numpy()
                print(f"[taxonomy_tables] generate_taxonomy_matrices case {gi}: tasks {sorted(mats)}")
    parents = random_forest(rng, BIG)
    tree = tree_of(parents, BIG)
    for lv in range(len(KEYS)):
        rec[f"big_parents_{lv}"] = parents[lv]
    dist = tree.build_distance_matrix(KEYS[0])
    alpha, beta, ur = SETTINGS[0]
    rec["big_dist"] = dist.numpy()
    rec["big_soft"] = build_taxonomy_smoothing_matrix(BIG[0], dist, alpha, beta, ur, roots_at(tree, KEYS[0])).numpy()
    path = os.path.join(OUT, "taxonomy_tables.npz")
    np.savez_compressed(path, **rec)
    print(f"[taxonomy_tables] {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
