"""numpy restatement of what the taxonomy smoothing tables stand for (linnaeus_amd.loss.TaxonomySmoothingTables, include/lnx.h:
LNX_CE_FORM_TAXONOMY, lnx_taxonomy_rows): the dense expansion of (anc, val), seeded forests, and the criterion in fp64.
Shared by tests/test_taxonomy_tables.py, tests/test_gpu_taxonomy_tables.py and the fixture's generator."""
import numpy as np

SETTINGS = ((0.1, 1.0, True), (0.3, 0.25, False), (0.1, 0.0, True), (0.0, 1.0, True), (0.1, 20.0, False))  # (alpha, beta, uniform_roots)


def heights(anc, rows=None):
    """k[i, c] for rows i: 0 at c == row, the first k in 1..D with anc[k-1, c] == anc[k-1, row] >= 0, D + 1 when there is none"""
    anc = np.asarray(anc)
    D, Cn = anc.shape
    rows = np.arange(Cn) if rows is None else np.asarray(rows, dtype=np.int64)
    k = np.full((len(rows), Cn), D + 1, np.int64)
    for j in range(D, 0, -1):  # downwards: the first height at which the chains meet is written last
        a = anc[j - 1]
        k[(a[rows][:, None] == a[None, :]) & (a[rows][:, None] >= 0)] = j
    k[np.arange(len(rows)), rows] = 0
    return k


def dense(anc, val, rows=None):
    """rows of the [C, C] soft-label matrix, in val's dtype (a gather: no arithmetic)"""
    val = np.asarray(val)
    rows = np.arange(val.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    return np.take_along_axis(val[rows], heights(anc, rows), 1)


def distances(anc, rows=None):
    """rows of the [C, C] distance matrix, fp32: 2k, inf where the chains never meet, 0 on the diagonal"""
    D = np.asarray(anc).shape[0]
    k = heights(anc, rows)
    return np.where(k > D, np.inf, 2.0 * k).astype(np.float32)


def random_forest(rng, ncls, p_orphan=0.15):
    """parents[l][i] = parent of class i of level l at level l + 1, -1 for none; the top level has no parents.  Guaranteed to
    hold: a parentless class and a class whose parent is parentless (a chain broken one level up) at every level that has
    room, and, at the finest level, a parent with exactly one child."""
    L_ = len(ncls)
    parents = []
    for lv in range(L_ - 1):
        p = rng.integers(0, ncls[lv + 1], ncls[lv])
        p[rng.random(ncls[lv]) < p_orphan] = -1
        p[0] = 0            # class 0 (the null class of the criterion tests) keeps a chain
        p[1] = -1           # a parentless class
        parents.append(p.astype(np.int64))
    for lv in range(L_ - 2):  # class 2 of level lv -> class 1 of level lv + 1, which has no parent: the chain breaks one level up
        if ncls[lv] > 2 and ncls[lv + 1] > 1:
            parents[lv][2] = 1
    if L_ > 1 and ncls[0] > 3 and ncls[1] > 2:  # parent 2 of the finest level gets exactly one child, class 3
        parents[0][parents[0] == 2] = 0
        parents[0][3] = 2
    parents.append(np.full(ncls[-1], -1, np.int64))
    return parents


def hierarchy_map(parents, keys):
    """the {child task: {child: parent}} map a TaxonomyTree is built from"""
    return {keys[lv]: {int(i): int(v) for i, v in enumerate(parents[lv]) if v >= 0} for lv in range(len(keys) - 1)}


class Tree:
    """the four members of the reference's TaxonomyTree that the table builders read"""

    def __init__(self, parents, keys, ncls):
        self.task_keys, self.num_classes = list(keys), dict(zip(keys, (int(c) for c in ncls)))
        self._parents = parents

    def get_nodes_at_level(self, task):
        return [(task, i) for i in range(self.num_classes.get(task, 0))]

    def get_parent(self, node):
        lv = self.task_keys.index(node[0])
        if lv + 1 >= len(self.task_keys) or self._parents[lv][node[1]] < 0:
            return None
        return (self.task_keys[lv + 1], int(self._parents[lv][node[1]]))


def soft_ce(logits, S, target, class_weight=None, ignore_index=None):
    """fp64 per-sample loss [B] and d loss[b] / d logits[b, :] of TaxonomyAwareLabelSmoothingCE.forward for soft rows S [B, C]"""
    x = np.asarray(logits, np.float64)
    S = np.asarray(S, np.float64)
    mx = x.max(1, keepdims=True)
    lse = mx + np.log(np.exp(x - mx).sum(1, keepdims=True))
    logp = x - lse
    loss = -(S * logp).sum(1)
    grad = np.exp(logp) * S.sum(1, keepdims=True) - S
    w = np.ones(len(x)) if class_weight is None else np.asarray(class_weight, np.float64)[target]
    if ignore_index is not None:
        w = np.where(np.asarray(target) == ignore_index, 0.0, w)
    return loss * w, grad * w[:, None]
