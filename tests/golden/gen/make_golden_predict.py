#!/usr/bin/env python3
"""Generate tests/golden/predict.npz from the reference's own enforce_hierarchical_consistency
(linnaeus/inference/postprocessing.py:14-171), unmodified, on its own TaxonomyTree (linnaeus/utils/taxonomy/taxonomy_tree.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_predict.py <linnaeus checkout>

`typus` is not installed and `linnaeus.inference` imports its whole serving stack, so postprocessing.py is loaded by file path into
the stand-in package _stubs/linnaeus_inference_standin (whose `artifacts` module holds the two names it imports as annotations), with
_stubs/typus supplying RankLevel (an Enum) and the two result records (dataclasses).  The tree is the real class, imported from the
checkout with the yacs / termcolor stand-ins.  Runs on CPU.  Writes numbers only:

  tree      four ranks taxa_L10 .. taxa_L40 with (7, 5, 4, 3) classes, class 0 the null of every rank (no parent, as
            vectorized_dataset_processor leaves it), `parent_<task>` = the hierarchy map as an array (-1 = none), `taxon_id_<task>`
  inputs    24 samples of seeded continuous fp32 logits, a bump on the class each scenario wants on top; `k` per sample (1, 3, 5; 5
            exceeds the 4 and 3 classes of the two coarse ranks).  Asserted free of ties, in the logits and in the fp32 probabilities.
  scenario  per sample: 0 fully consistent; 1 / 2 / 3 inconsistent at taxa_L30 / L20 / L10; 4 / 5 / 6 / 7 null top-1 at
            taxa_L40 / L30 / L20 / L10 (5-7: a null top-1 under a non-null parent)
  raw       the handler's recipe (handler.py:195-210: torch.softmax, torch.topk, .item()) -> `raw_ids`, `raw_probs`, `raw_count`
  final     enforce_hierarchical_consistency on that -> `ids`, `probs`, `count`, all [B, T, 5] / [B, T] padded with (-1, 0), task
            axis finest first
"""
import importlib.util
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "inference", "postprocessing.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(HERE, "_stubs"), REF]
sys.dont_write_bytecode = True

import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

warnings.filterwarnings("ignore")
logging.disable(logging.CRITICAL)

import linnaeus_inference_standin  # noqa: E402,F401
from typus.constants import RankLevel  # noqa: E402
from typus.models.classification import HierarchicalClassificationResult, TaskPrediction  # noqa: E402

from linnaeus.utils.taxonomy.taxonomy_tree import TaxonomyTree  # noqa: E402

spec = importlib.util.spec_from_file_location("linnaeus_inference_standin.postprocessing", os.path.join(REF, "linnaeus", "inference", "postprocessing.py"))
post = importlib.util.module_from_spec(spec)
sys.modules[spec.name] = post
spec.loader.exec_module(post)

SEED = 20240902
KEYS = ["taxa_L10", "taxa_L20", "taxa_L30", "taxa_L40"]  # finest first
CLASSES = {"taxa_L10": 7, "taxa_L20": 5, "taxa_L30": 4, "taxa_L40": 3}
HIERARCHY = {  # child task -> {child class: parent class in the next task}; the null class 0 has no entry
    "taxa_L10": {1: 1, 2: 1, 3: 2, 4: 3, 5: 4, 6: 4},
    "taxa_L20": {1: 1, 2: 2, 3: 3, 4: 3},
    "taxa_L30": {1: 1, 2: 1, 3: 2},
}
KMAX = 5
# top-1 class wanted at (L40, L30, L20, L10) per scenario
SCENARIOS = {
    0: [(1, 1, 1, 1), (1, 1, 1, 2), (1, 2, 2, 3), (2, 3, 3, 4), (2, 3, 4, 6)],
    1: [(2, 1, 1, 1), (1, 3, 3, 4)],
    2: [(1, 1, 2, 3), (2, 3, 1, 1)],
    3: [(1, 1, 1, 3), (2, 3, 4, 1)],
    4: [(0, 1, 1, 1), (0, 3, 4, 5)],
    5: [(1, 0, 1, 1), (2, 0, 0, 0)],
    6: [(1, 1, 0, 1), (2, 3, 0, 5)],
    7: [(1, 1, 1, 0), (2, 3, 4, 0)],
}


def rank_of(key):
    return RankLevel(int(key.split("_L")[-1]))


def main():
    tree = TaxonomyTree(HIERARCHY, KEYS, CLASSES)
    taxon_id = {k: np.array([1000 * rank_of(k).value + 7 * i + 3 for i in range(CLASSES[k])], dtype=np.int64) for k in KEYS}
    class_maps = SimpleNamespace(
        null_taxon_ids={rank_of(k): int(taxon_id[k][0]) for k in KEYS},
        taxon_id_to_idx={rank_of(k): {int(t): i for i, t in enumerate(taxon_id[k])} for k in KEYS},
        idx_to_taxon_id={rank_of(k): {i: int(t) for i, t in enumerate(taxon_id[k])} for k in KEYS},
        num_classes_per_rank={rank_of(k): CLASSES[k] for k in KEYS},
    )
    taxonomy_data = SimpleNamespace(taxonomy_tree=tree)

    wanted, scenario = [], []
    for s, tops in SCENARIOS.items():
        for tp in tops:
            wanted.append(tp)
            scenario.append(s)
    wanted += [SCENARIOS[0][0], SCENARIOS[2][0], SCENARIOS[4][0], SCENARIOS[5][0], SCENARIOS[7][0]]  # again, under another k
    scenario += [0, 2, 4, 5, 7]
    B, T = len(wanted), len(KEYS)
    assert B == 24
    k = np.array([(5, 3, 1)[b % 3] for b in range(B)], dtype=np.int32)
    g = torch.Generator().manual_seed(SEED)
    logits = {}
    for t, key in enumerate(KEYS):
        x = torch.randn(B, CLASSES[key], generator=g)
        x[torch.arange(B), torch.tensor([w[T - 1 - t] for w in wanted])] += 6.0
        assert all(len(set(row.tolist())) == row.numel() for row in x), "tied logits"
        logits[key] = x

    shape = (B, T, KMAX)
    rec = {"task_keys": np.array(KEYS), "num_classes": np.array([CLASSES[k_] for k_ in KEYS]), "k": k, "scenario": np.array(scenario, dtype=np.int32),
           "null_index": np.zeros(T, dtype=np.int32)}
    for key in KEYS:
        rec[f"logits_{key}"] = logits[key].numpy()
        rec[f"taxon_id_{key}"] = taxon_id[key]
    for key in KEYS[:-1]:
        rec[f"parent_{key}"] = np.array([HIERARCHY[key].get(c, -1) for c in range(CLASSES[key])], dtype=np.int32)
        for c in range(CLASSES[key]):  # the array is the tree's own get_parent
            node = tree.get_parent((key, c))
            assert (node[1] if node is not None else -1) == rec[f"parent_{key}"][c]
    out = {n: (np.full(shape, -1, dtype=np.int64), np.zeros(shape, dtype=np.float64), np.zeros((B, T), dtype=np.int32)) for n in ("raw", "final")}
    changed = 0
    for b in range(B):
        tasks = []
        for key in KEYS:  # handler.py:190-216
            probs = torch.softmax(logits[key][b], dim=-1)
            actual_k = min(int(k[b]), CLASSES[key])
            top_p, top_i = torch.topk(probs, k=actual_k)
            assert len(set(probs.tolist())) == probs.numel(), "tied probabilities"
            preds = [(class_maps.idx_to_taxon_id[rank_of(key)][top_i[j].item()], top_p[j].item()) for j in range(actual_k)]
            tasks.append(TaskPrediction(rank_level=rank_of(key), temperature=1.0, predictions=preds))
        tasks.sort(key=lambda t_: t_.rank_level.value, reverse=True)  # handler.py:218
        raw = HierarchicalClassificationResult(taxonomy_context=None, tasks=tasks, subtree_roots=None)
        final = post.enforce_hierarchical_consistency(raw, taxonomy_data, class_maps)
        for name, res in (("raw", raw), ("final", final)):
            ids, probs, count = out[name]
            for tp in res.tasks:
                t = KEYS.index(f"taxa_L{tp.rank_level.value}")
                count[b, t] = len(tp.predictions)
                for j, (tid, p) in enumerate(tp.predictions):
                    ids[b, t, j], probs[b, t, j] = tid, p
        changed += int(not (np.array_equal(out["raw"][0][b], out["final"][0][b]) and np.array_equal(out["raw"][1][b], out["final"][1][b])))
    rec["raw_ids"], rec["raw_probs"], rec["raw_count"] = out["raw"]
    rec["ids"], rec["probs"], rec["count"] = out["final"]
    assert changed == sum(s != 0 for s in scenario), (changed, scenario)  # every scenario but "consistent" changes something
    path = os.path.join(REPO, "tests", "golden", "predict.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes;", changed, "of", B, "samples changed by the consistency pass")
    for b in range(B):
        print(b, "scenario", scenario[b], "k", k[b], "count", rec["count"][b].tolist(), "top ids", rec["ids"][b, :, 0].tolist())


if __name__ == "__main__":
    main()
