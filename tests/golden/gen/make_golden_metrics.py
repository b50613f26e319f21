#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz from the reference's own metric bookkeeping (linnaeus/utils/metrics/chain_accuracy.py
compute_chain_accuracy_vectorized / compute_partial_chain_accuracy_vectorized, linnaeus/utils/metrics/tracker.py
MetricsTracker._update_phase_batch).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_metrics.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/ and runs on CPU.  Writes numbers only:

  inputs    NB batches of B samples over four tasks (taxa_L10 .. taxa_L40, 20 / 80 / 300 / 1000 classes): seeded continuous fp32
            logits (no ties, so nothing the reference returns depends on tie order) nudged towards the target so that the
            accuracies are neither 0 nor 1, integer targets with null (0) labels -- some samples all null --, per-sample losses
  chain     per batch, the two chain functions' return values, for index targets and for one-hot targets
  tracker   the accumulators of a MetricsTracker after _update_phase_batch over the NB batches with one-hot targets, null tracking
            on for taxa_L10 and taxa_L30.  The tracker is made with MetricsTracker.__new__ and given exactly the attributes
            _update_phase_batch touches: its constructor wants an OpsSchedule and the full experiment config, none of which the
            batch update reads.  `loss_components` carries the batch-mean task losses and the raw per-sample losses, as
            validation.py does.
"""
import os
import sys
from collections import defaultdict
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "utils", "metrics", "tracker.py")):
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

from linnaeus.utils.metrics.chain_accuracy import compute_chain_accuracy_vectorized, compute_partial_chain_accuracy_vectorized  # noqa: E402
from linnaeus.utils.metrics.tracker import MetricsTracker  # noqa: E402

SEED = 20240611
TASKS = [("taxa_L10", 20), ("taxa_L20", 80), ("taxa_L30", 300), ("taxa_L40", 1000)]
NB, B = 3, 32
NULL_TASKS = ["taxa_L10", "taxa_L30"]
PHASE = "val"


def make_batch(g):
    logits, targets, losses = {}, {}, {}
    null_p = torch.rand(B, generator=g)
    for i, (t, c) in enumerate(TASKS):
        y = torch.randint(1, c, (B,), generator=g)
        y[torch.rand(B, generator=g) < 0.15 + 0.1 * i] = 0  # null labels, more of them at the finer ranks
        y[null_p < 0.08] = 0  # samples that are null at every rank
        x = torch.randn(B, c, generator=g)
        x[torch.arange(B), y] += 3.5 + 0.5 * i  # right often, not always; still continuous
        logits[t], targets[t] = x, y
        losses[t] = torch.rand(B, generator=g) * 3.0
    return logits, targets, losses


def bare_tracker():
    tr = MetricsTracker.__new__(MetricsTracker)
    tr.config = SimpleNamespace(TRAIN=SimpleNamespace(PHASE1_MASK_NULL_LOSS=False), DEBUG=SimpleNamespace(VALIDATION_METRICS=False))
    tr.null_tracking_enabled = True
    tr.null_tracking_tasks = list(NULL_TASKS)
    tr.phase_metrics = {PHASE: {}}
    tr.phase_subset_metrics = {PHASE: {}}
    tr.chain_correct, tr.chain_total = {PHASE: 0}, {PHASE: 0}
    tr.partial_chain_correct, tr.partial_chain_total = {PHASE: 0}, {PHASE: 0}
    tr.partial_task_sums = {PHASE: defaultdict(lambda: defaultdict(float))}
    tr.partial_task_counts = {PHASE: defaultdict(lambda: defaultdict(int))}
    tr.partial_null_sums = {PHASE: defaultdict(lambda: defaultdict(float))}
    tr.partial_null_counts = {PHASE: defaultdict(lambda: defaultdict(int))}
    tr.partial_non_null_sums = {PHASE: defaultdict(lambda: defaultdict(float))}
    tr.partial_non_null_counts = {PHASE: defaultdict(lambda: defaultdict(int))}
    return tr


def main():
    g = torch.Generator().manual_seed(SEED)
    keys = [t for t, _ in TASKS]
    rec = {"task_keys": np.array(keys), "num_classes": np.array([c for _, c in TASKS]), "null_tasks": np.array(NULL_TASKS), "n_batches": np.array(NB)}
    tr = bare_tracker()
    chain, partial, chain_1h, partial_1h = [], [], [], []
    for n in range(NB):
        logits, targets, losses = make_batch(g)
        onehot = {t: torch.nn.functional.one_hot(targets[t], c).float() for t, c in TASKS}
        for t in keys:
            rec[f"logits_{n}_{t}"] = logits[t].numpy()
            rec[f"target_{n}_{t}"] = targets[t].numpy()
            rec[f"loss_{n}_{t}"] = losses[t].numpy()
        outs = [logits[t] for t in keys]
        chain.append(compute_chain_accuracy_vectorized(outs, [targets[t] for t in keys]))
        partial.append(compute_partial_chain_accuracy_vectorized(outs, [targets[t] for t in keys]))
        chain_1h.append(compute_chain_accuracy_vectorized(outs, [onehot[t] for t in keys]))
        partial_1h.append(compute_partial_chain_accuracy_vectorized(outs, [onehot[t] for t in keys]))
        comps = {"tasks": {t: float(losses[t].mean()) for t in keys}, "raw_per_sample_losses": {t: losses[t] for t in keys}}
        rec[f"task_loss_mean_{n}"] = np.array([comps["tasks"][t] for t in keys], dtype=np.float64)
        tr._update_phase_batch(PHASE, logits, onehot, comps, {})
    rec["chain"], rec["partial"] = np.array(chain, dtype=np.float64), np.array(partial, dtype=np.float64)
    rec["chain_onehot"], rec["partial_onehot"] = np.array(chain_1h, dtype=np.float64), np.array(partial_1h, dtype=np.float64)
    rec["tr_chain"] = np.array([tr.chain_correct[PHASE], tr.chain_total[PHASE], tr.partial_chain_correct[PHASE], tr.partial_chain_total[PHASE]], dtype=np.float64)
    for kind in ("acc1", "acc3", "loss"):
        rec[f"tr_task_sums_{kind}"] = np.array([tr.partial_task_sums[PHASE][t][kind] for t in keys], dtype=np.float64)
        rec[f"tr_task_counts_{kind}"] = np.array([tr.partial_task_counts[PHASE][t][kind] for t in keys], dtype=np.int64)
    for name, sums, counts in (("null", tr.partial_null_sums, tr.partial_null_counts), ("non_null", tr.partial_non_null_sums, tr.partial_non_null_counts)):
        for kind in ("acc1", "loss"):
            rec[f"tr_{name}_sums_{kind}"] = np.array([sums[PHASE][t][kind] for t in NULL_TASKS], dtype=np.float64)
            rec[f"tr_{name}_counts_{kind}"] = np.array([counts[PHASE][t][kind] for t in NULL_TASKS], dtype=np.int64)
    out = os.path.join(REPO, "tests", "golden", "metrics.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")
    print("chain", chain, "partial", partial, "tracker", rec["tr_chain"])


if __name__ == "__main__":
    main()
