"""Plain numpy restatement of lnx_metrics_update's table update (include/lnx.h): the bookkeeping of the reference's
MetricsTracker._update_phase_batch (utils/metrics/tracker.py:609-937) and chain_accuracy.py:143-166,299-344 as integer counters and
float64 sums.  Test infrastructure (like dwconv_ref.py): written from the stated rules with a stable sort, sharing no code with the
kernel or with linnaeus_amd.metrics."""
import numpy as np

# counts layout (mirrors the LNX_METRICS_* enums)
CHAIN_N, CHAIN_CORRECT, PARTIAL_N, PARTIAL_CORRECT, SUBSET_OOR = 0, 1, 2, 3, 4
HEAD, TASK_STRIDE, SUM_STRIDE = 8, 8, 4
N, CORRECT1, CORRECT3, NULL_N, NULL_CORRECT1, NONNULL_N, NONNULL_CORRECT1, LOSS_N = range(8)
SUM_LOSS, SUM_NULL_LOSS, SUM_NONNULL_LOSS = range(3)


def task_off(t):
    return HEAD + TASK_STRIDE * t


def subset_off(n_tasks, n_bins0, s):
    return task_off(n_tasks) + (2 * n_tasks * n_bins0 if s else 0)


def table_sizes(n_tasks, n_bins0=0, n_bins1=0):
    return subset_off(n_tasks, n_bins0, 1) + 2 * n_tasks * n_bins1, SUM_STRIDE * n_tasks


def order(row):
    """Indices of `row` by (value descending, index ascending), every NaN in front of every number."""
    row = np.asarray(row, dtype=np.float64)
    nan = np.isnan(row)
    return np.concatenate([np.flatnonzero(nan), np.flatnonzero(~nan)[np.argsort(-row[~nan], kind="stable")]])


def update(counts, sums, logits, targets, num_classes=None, is_null=None, losses=None, subset_ids=(), n_bins=()):
    """Adds one batch to counts (int64) / sums (float64) in place.  logits: per task [B, >= C] (any float dtype, converted exactly to
    float64); targets: per task int [B]; is_null / losses: per task [B] or None; subset_ids / n_bins: up to two id vectors."""
    T = len(logits)
    B = len(targets[0])
    right = np.zeros((B, T), dtype=bool)
    gts = np.stack([np.asarray(t, dtype=np.int64) for t in targets], axis=1)
    for t in range(T):
        C = int(num_classes[t]) if num_classes is not None else logits[t].shape[1]
        x = np.asarray(logits[t], dtype=np.float64)[:, :C]
        tg = gts[:, t]
        null = np.asarray(is_null[t]).astype(bool) if is_null is not None and is_null[t] is not None else tg == 0
        c = counts[task_off(t): task_off(t) + TASK_STRIDE]
        for b in range(B):
            top = order(x[b])[:3]
            c1 = top[0] == tg[b]
            c3 = c1 if C < 3 else bool((top == tg[b]).any())
            right[b, t] = c1
            c[N] += 1
            c[CORRECT1] += c1
            c[CORRECT3] += c3
            c[NULL_N if null[b] else NONNULL_N] += 1
            c[NULL_CORRECT1 if null[b] else NONNULL_CORRECT1] += c1
        if losses is not None and losses[t] is not None:
            ls = np.asarray(losses[t], dtype=np.float64)
            s = sums[SUM_STRIDE * t: SUM_STRIDE * t + SUM_STRIDE]
            s[SUM_LOSS] += ls.sum()
            s[SUM_NULL_LOSS] += ls[null].sum()
            s[SUM_NONNULL_LOSS] += ls[~null].sum()
            c[LOSS_N] += B
    counts[CHAIN_N] += B
    counts[CHAIN_CORRECT] += int(right.all(axis=1).sum())
    for b in range(B):
        non_null = np.flatnonzero(gts[b] != 0)
        if len(non_null):
            counts[PARTIAL_N] += 1
            counts[PARTIAL_CORRECT] += bool(right[b, : non_null[-1] + 1].all())
    nb0 = n_bins[0] if len(n_bins) and subset_ids[0] is not None else 0
    for s, ids in enumerate(subset_ids):
        if ids is None:
            continue
        base = subset_off(T, nb0, s)
        for b, i in enumerate(np.asarray(ids, dtype=np.int64)):
            if i < 0 or i >= n_bins[s]:
                counts[SUBSET_OOR + s] += 1
                continue
            for t in range(T):
                counts[base + 2 * (t * n_bins[s] + i)] += 1
                counts[base + 2 * (t * n_bins[s] + i) + 1] += right[b, t]
    return counts, sums


def fresh(n_tasks, n_bins0=0, n_bins1=0):
    nc, ns = table_sizes(n_tasks, n_bins0, n_bins1)
    return np.zeros(nc, dtype=np.int64), np.zeros(ns, dtype=np.float64)
