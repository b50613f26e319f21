"""Plain numpy (float64) restatement of lnx_predict: what the reference's inference handler does after the forward
(linnaeus/inference/handler.py:186-228) followed by enforce_hierarchical_consistency (linnaeus/inference/postprocessing.py:64-154),
with the order the library defines where torch leaves it open.

  order    value descending, then index ascending, NaN above every number: one stable sort (the order of tests/metrics_ref.py)
  probs    exp(x - max) / sum exp(x - max) in float64 over the whole row (handler.py:196 softmax); a NaN makes the row NaN
  raw      the first min(k_b, C) entries of the order (handler.py:200-202)
  chain    coarsest task first (postprocessing.py:37), keeping the consistent node of the task above (:43):
             the coarsest keeps its raw list, its node is its top-1 (:153-154)
             (a) node above == that task's null index                      -> flag 1 (:121)
             (b) else parent[top-1] != node above (None / -1 is different)  -> flag 2 (:133-134)
             (c) else kept, node = top-1                                    -> flag 0 (:148)
           flagged with a null index: the list becomes [(null, 1.0)], node = null (:124-126, :141-143);
           flagged without one: the list stays, node = top-1 (:128, :145)
Tasks are given finest first, as the kernel takes them.  Entries at or beyond count are (-1, 0).
"""
import numpy as np


def order(row):
    """Indices of row in (value descending, index ascending, NaN first) order."""
    row = np.asarray(row, dtype=np.float64)
    nan = np.isnan(row)
    neg = np.where(nan, 0.0, -row) + 0.0  # (-0.0 + 0.0 = +0.0: the two zeros tie)
    return np.lexsort((np.arange(row.size), neg, ~nan))  # the last key is the first criterion; equal keys keep the index order


def softmax(row):
    row = np.asarray(row, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(row - np.max(row))  # np.max hands a NaN on
        return e / e.sum()


def predict(logits, parents, K, null_index=0, id_maps=None, k_per_sample=None, consistency=True):
    """logits: per task [B, C] (finest first); parents: per task int [C] or None (the coarsest); null_index: an int or per task
    int / None.  Returns ids int64 [B, T, K], probs float64 [B, T, K], count int32 [B, T], flags int32 [B, T]."""
    T, B = len(logits), np.asarray(logits[0]).shape[0]
    nulls = list(null_index) if isinstance(null_index, (list, tuple)) else [null_index] * T
    ids = np.full((B, T, K), -1, dtype=np.int64)
    probs = np.zeros((B, T, K), dtype=np.float64)
    count = np.zeros((B, T), dtype=np.int32)
    flags = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        kb = K if k_per_sample is None else min(max(int(k_per_sample[b]), 1), K)
        above = above_null = None
        for t in range(T - 1, -1, -1):
            row = np.asarray(logits[t][b], dtype=np.float64)
            n = min(kb, row.size)
            top = order(row)[:n]
            p = softmax(row)[top]
            result = list(zip(top.tolist(), p.tolist()))
            c = int(top[0])
            flag = 0
            if consistency and t < T - 1:
                if above_null is not None and above == above_null:
                    flag = 1
                elif int(parents[t][c]) != above:
                    flag = 2
            if flag and nulls[t] is not None:
                result = [(int(nulls[t]), 1.0)]
                above = int(nulls[t])
            else:
                above = c
            above_null = nulls[t]
            flags[b, t] = flag
            count[b, t] = len(result)
            for j, (cls, pr) in enumerate(result):
                ids[b, t, j] = cls if id_maps is None or id_maps[t] is None else int(id_maps[t][cls])
                probs[b, t, j] = pr
    return ids, probs, count, flags
