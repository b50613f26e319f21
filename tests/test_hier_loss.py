"""The fused hierarchical loss without a GPU: a NumPy restatement of its semantics (hier_ref, the yardstick of
tests/test_gpu_hier_loss.py) against the reference's own numbers in tests/golden/hier_loss.npz and hier_loss_soft.npz, the
class-weight powers the host hands to the kernel, and the argument refusals of both C-ABI entry points (checked before any launch)."""
import ctypes as C
import itertools
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest

from linnaeus_amd import _lib as L
from linnaeus_amd.loss import class_weight_powers

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")

# mode -> (prob, PHASE1_MASK_NULL_LOSS, is_validation, class weights given); the fixtures were recorded with CLASS.TRAIN = True, CLASS.VAL = False
MODES = {"sched1": (1.0, False, False, True), "sched0": (0.0, False, False, True), "phase1": (1.0, True, False, True), "val": (0.0, False, True, True),
         "sched0_nocw": (0.0, False, False, False)}
SOFT_MODES = ("sched1", "sched0", "phase1", "val")


def hier_ref(logits, targets, soft, weights, prob, *, smoothing=None, crit_weight=None, ignore_index=None, cw=None, p_cw=None, p_w=None, draws=None,
             mask_mul=False, go=1.0):
    """The semantics of lnx_hier_loss_fwd / lnx_hier_loss_bwd in float64.  Per task (lists in task order): logits [B, C]; targets [B] integers
    or [B, C] floats; soft [C, C] or None (one-hot with uniform smoothing[t]); crit_weight [C] or None; ignore_index or None; cw = class-weight
    vector or None with the powers p_cw / p_w; draws [B] uniform numbers (read for 0 < prob < 1)."""
    T = len(logits)
    res = dict(raw=[], keep=[], null=[], raw_mean=[], masked_mean=[], weighted=[], nvalid=[], grads=[], scale=[])
    for t in range(T):
        x = np.asarray(logits[t], dtype=np.float64)
        B, Cn = x.shape
        y = np.asarray(targets[t])
        if y.ndim == 2:
            cls = y.argmax(1)  # numpy's first-maximum rule is torch's
            null = y[:, 0] > 0.5
        else:
            cls = y.astype(np.int64)
            null = cls == 0
        bad = (cls < 0) | (cls >= Cn)
        safe = np.where(bad, 0, cls)
        if soft[t] is not None:
            S = np.asarray(soft[t], dtype=np.float64)[safe]
        else:
            eps = float(smoothing[t]) if smoothing is not None else 0.0
            S = np.full((B, Cn), eps / Cn)
            S[np.arange(B), safe] += 1.0 - eps
        mx = x.max(1, keepdims=True)
        lse = (mx + np.log(np.exp(x - mx).sum(1, keepdims=True)))[:, 0]
        ss = S.sum(1)
        cwc = np.ones(B) if crit_weight is None or crit_weight[t] is None else np.asarray(crit_weight[t], dtype=np.float64)[safe]
        ign = np.zeros(B, bool) if ignore_index is None or ignore_index[t] is None or ignore_index[t] < 0 else cls == ignore_index[t]
        raw = np.where(bad, np.nan, np.where(ign, 0.0, cwc * (lse * ss - (S * x).sum(1))))
        gcrit = np.where(bad | ign, 0.0, cwc)
        if prob >= 1.0:
            keep = np.ones(B, bool)
        elif prob <= 0.0:
            keep = ~null
        else:
            keep = ~null | (np.asarray(draws[t], dtype=np.float32) < np.float32(prob))
        masked = raw * keep if mask_mul else np.where(keep, raw, 0.0)
        pc, pw = (0, 0) if cw is None or cw[t] is None else (p_cw[t], p_w[t])
        if pw:
            v = np.asarray(cw[t], dtype=np.float64)
            if y.ndim == 2:
                scw = (y.astype(np.float64) * v[None, :Cn]).sum(1)
            else:
                scw = np.where(cls < len(v), v[np.clip(cls, 0, len(v) - 1)], 1.0)
        else:
            scw = np.ones(B)
        nvalid = float(B) if mask_mul else float((masked != 0).sum())
        den = max(nvalid, 1e-6)
        scale = float(weights[t]) / den
        coef = keep * scw ** pw * gcrit
        p = np.exp(x - lse[:, None])
        grad = np.where((coef == 0)[:, None], 0.0, go * scale * coef[:, None] * (p * ss[:, None] - S))
        res["raw"].append(raw), res["keep"].append(keep), res["null"].append(null)
        res["raw_mean"].append(raw.mean()), res["masked_mean"].append((masked * scw ** pc).mean())
        res["weighted"].append((masked * scw ** pw).sum() / den * float(weights[t]))
        res["nvalid"].append(int(nvalid)), res["grads"].append(grad), res["scale"].append(scale)
    res["total"] = float(np.sum(res["weighted"]))
    res["null_total"] = int(sum(n.sum() for n in res["null"]))
    res["null_included"] = int(sum((n & k).sum() for n, k in zip(res["null"], res["keep"])))
    res["inclusion_percentage"] = res["null_included"] * 100.0 / max(res["null_total"], 1)
    return res


def fixture_case(name, mode):
    """inputs of one recorded mode as hier_ref takes them, and the npz with the reference's outputs"""
    z = np.load(os.path.join(GOLDEN, name))
    tasks = [str(t) for t in z["tasks"]]
    prob, phase1, val, use_cw = MODES[mode]
    cfg = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=phase1), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=True, VAL=False))))
    cwd = {t: {i: float(z[f"cw_{t}"][i]) for i in range(0, int(c), 2)} for t, c in zip(tasks, z["classes"])} if use_cw else None
    powers = [class_weight_powers(NS(class_weights=cwd), cfg, val, t) for t in tasks]
    eff = 1.0 if val else (0.0 if phase1 else prob)
    kw = dict(cw=[z[f"cw_{t}"] if use_cw else None for t in tasks], p_cw=[p[0] for p in powers], p_w=[p[1] for p in powers], mask_mul=phase1 and not val)
    args = ([z[f"logits_{t}"] for t in tasks], [z[f"target_{t}"] for t in tasks], [z[f"soft_{t}"] for t in tasks], z["task_weights"], eff)
    return z, tasks, cfg, cwd, args, kw


def check_against_fixture(z, tasks, mode, total, weighted, raw_mean, masked_mean, grads):
    """the tolerances of tests/test_loss.py: totals and components rtol 2e-5, gradients rtol 2e-4 / atol 2e-6"""
    assert abs(total - float(z[f"{mode}_total"])) <= 2e-5 * abs(float(z[f"{mode}_total"])), (total, float(z[f"{mode}_total"]))
    np.testing.assert_allclose(weighted, z[f"{mode}_weighted"], rtol=2e-5)
    np.testing.assert_allclose(raw_mean, z[f"{mode}_raw_mean"], rtol=2e-5)
    np.testing.assert_allclose(masked_mean, z[f"{mode}_masked_mean"], rtol=2e-5)
    for t, g in zip(tasks, grads):
        np.testing.assert_allclose(g, z[f"{mode}_grad_{t}"], rtol=2e-4, atol=2e-6)


@pytest.mark.parametrize("mode", list(MODES))
def test_restatement_matches_the_reference(mode):
    z, tasks, _, _, args, kw = fixture_case("hier_loss.npz", mode)
    r = hier_ref(*args, **kw)
    check_against_fixture(z, tasks, mode, r["total"], r["weighted"], r["raw_mean"], r["masked_mean"], r["grads"])


@pytest.mark.parametrize("mode", SOFT_MODES)
def test_restatement_matches_the_reference_on_soft_targets(mode):
    z, tasks, _, _, args, kw = fixture_case("hier_loss_soft.npz", mode)
    r = hier_ref(*args, **kw)
    check_against_fixture(z, tasks, mode, r["total"], r["weighted"], r["raw_mean"], r["masked_mean"], r["grads"])


def test_soft_fixture_holds_the_rows_it_is_for():
    z = np.load(os.path.join(GOLDEN, "hier_loss_soft.npz"))
    for t, c in zip(z["tasks"], z["classes"]):
        y = z[f"target_{t}"]
        assert y.shape == (16, int(c)) and y.dtype == np.float32
        null = y[:, 0] > 0.5
        assert 0 < null.sum() < 16
        assert ((y == y.max(1, keepdims=True)).sum(1) == 1).all()  # tie-free maximum
        assert (y.argmax(1) != 0).any() and ((y[:, 0] > 0) & ~null).any()


# (p_cw, p_w) for a task that HAS class weights, counted by reading the composed path in linnaeus_amd/loss.py:
#   apply_loss_masking multiplies once (`if class_weights is not None`) -- skipped by the PHASE1 training branch, which masks by itself;
#   weighted_hierarchical_loss multiplies once more under CLASS.TRAIN (training) / CLASS.VAL (validation);  -> masked_tasks is logged here
#   GradientWeighting.forward multiplies once more (`if self.class_weights and t in self.class_weights`).   -> the weighted loss
# key: (is_validation, PHASE1_MASK_NULL_LOSS, CLASS.TRAIN, CLASS.VAL)
POWERS = {
    (False, False, True, True): (2, 3), (False, False, True, False): (2, 3), (False, False, False, True): (1, 2), (False, False, False, False): (1, 2),
    (False, True, True, True): (1, 2), (False, True, True, False): (1, 2), (False, True, False, True): (0, 1), (False, True, False, False): (0, 1),
    (True, False, True, True): (2, 3), (True, False, True, False): (1, 2), (True, False, False, True): (2, 3), (True, False, False, False): (1, 2),
    (True, True, True, True): (2, 3), (True, True, True, False): (1, 2), (True, True, False, True): (2, 3), (True, True, False, False): (1, 2),
}


def test_class_weight_powers_table():
    for val, phase1, ctrain, cval in itertools.product((False, True), repeat=4):
        cfg = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=phase1), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=ctrain, VAL=cval))))
        with_cw = NS(class_weights={"taxa_L10": {0: 2.0}})
        assert class_weight_powers(with_cw, cfg, val, "taxa_L10") == POWERS[(val, phase1, ctrain, cval)], (val, phase1, ctrain, cval)
        assert class_weight_powers(with_cw, cfg, val, "taxa_L20") == (0, 0)  # a task the dict does not name
        for none in (None, {}):
            assert class_weight_powers(NS(class_weights=none), cfg, val, "taxa_L10") == (0, 0)
    # no config at all: no PHASE1 branch, and the CLASS switch defaults to True (the composed path's `except`)
    assert class_weight_powers(NS(class_weights={"taxa_L10": {0: 2.0}}), None, False, "taxa_L10") == (2, 3)
    assert class_weight_powers(NS(class_weights={"taxa_L10": {0: 2.0}}), NS(TRAIN=NS()), True, "taxa_L10") == (2, 3)


def _valid_args():
    fake = C.c_void_p(0x1000)  # never dereferenced: every case below is refused on the host
    a = L.HierLossArgs()
    a.dtype, a.B, a.n_tasks, a.prob, a.mask_mul = L.F32, 4, 2, 1.0, 0
    a.draws, a.weights, a.ws, a.out, a.counts = None, fake, fake, fake, fake
    for t in range(2):
        k = a.task[t]
        k.logits, k.ld, k.C, k.target, k.soft, k.smoothing, k.ignore_index = fake, 8, 5, fake, fake, 0.0, -1
        k.class_weight, k.n_cw, k.p_cw, k.p_w, k.dlogits, k.ldd = fake, 5, 1, 2, fake, 8
    return a


def _set(path, value):
    def f(a):
        obj = a
        for p in path[:-1]:
            obj = obj[p] if isinstance(p, int) else getattr(obj, p)
        setattr(obj, path[-1], value)
    return f


REFUSALS = [
    (_set(("n_tasks",), 0), b"n_tasks"), (_set(("n_tasks",), 9), b"n_tasks"), (_set(("B",), 0), b"B=0"), (_set(("B",), -3), b"B=-3"),
    (_set(("dtype",), 2), b"dtype"), (_set(("ws",), None), b"ws"), (_set(("out",), None), b"out"), (_set(("counts",), None), b"counts"),
    (_set(("weights",), None), b"weights"), (_set(("prob",), 0.5), b"draws"),
    (_set(("task", 1, "C"), 0), b"C=0"), (_set(("task", 1, "ld"), 4), b"ld=4"), (_set(("task", 0, "logits"), None), b"logits"),
    (_set(("task", 0, "target"), None), b"target"), (_set(("task", 0, "soft_target"), 0x1000), b"target"),
    (_set(("task", 1, "smoothing"), 1.0), b"smoothing"), (_set(("task", 1, "smoothing"), -0.1), b"smoothing"),
    (_set(("task", 0, "p_cw"), 4), b"p_cw"), (_set(("task", 0, "p_w"), -1), b"p_w"), (_set(("task", 0, "p_w"), 0), b"p_cw"),
    (_set(("task", 1, "class_weight"), None), b"class_weight"), (_set(("task", 1, "ldd"), 4), b"ldd=4"),
]


@pytest.mark.parametrize("entry", ["lnx_hier_loss_fwd", "lnx_hier_loss_bwd"])
def test_entry_points_refuse_bad_arguments_before_any_launch(entry):
    lib = L.lib()
    fake = C.c_void_p(0x1000)
    call = (lambda a: lib.lnx_hier_loss_fwd(a, None)) if entry == "lnx_hier_loss_fwd" else (lambda a: lib.lnx_hier_loss_bwd(a, fake, None))
    assert call(None) != 0 and b"NULL arguments" in lib.lnx_last_error()
    for i, (spoil, word) in enumerate(REFUSALS):
        a = _valid_args()
        spoil(a)
        assert call(C.byref(a)) != 0, i
        msg = lib.lnx_last_error()
        assert entry.encode() in msg and word in msg, (i, msg)
    # soft targets: their own leading dimension, and a class-weight vector that covers every class
    for spoil, word in ((_set(("task", 0, "ldt"), 3), b"ldt=3"), (_set(("task", 0, "n_cw"), 4), b"n_cw=4")):
        a = _valid_args()
        a.task[0].target, a.task[0].soft_target, a.task[0].ldt = None, 0x1000, 5
        spoil(a)
        assert call(C.byref(a)) != 0 and word in lib.lnx_last_error(), lib.lnx_last_error()
    if entry == "lnx_hier_loss_bwd":
        a = _valid_args()
        assert lib.lnx_hier_loss_bwd(C.byref(a), None, None) != 0 and b"go_dev" in lib.lnx_last_error()
        a.task[0].dlogits = a.task[1].dlogits = None
        assert lib.lnx_hier_loss_bwd(C.byref(a), fake, None) != 0 and b"dlogits" in lib.lnx_last_error()


def test_python_refusals_need_no_gpu():
    """what FusedHierarchicalLoss refuses at construction, by name"""
    import torch

    from linnaeus_amd.loss import FusedHierarchicalLoss, GradientWeighting, TaxonomyAwareLabelSmoothingCE

    gw = GradientWeighting(["taxa_L10"], None, "static")
    with pytest.raises(L.LnxError, match="MSELoss"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": torch.nn.MSELoss()}, gw)
    with pytest.raises(L.LnxError, match="reduction"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": torch.nn.CrossEntropyLoss()}, gw)
    with pytest.raises(L.LnxError, match="class weight"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": torch.nn.CrossEntropyLoss(reduction="none", weight=torch.ones(3))}, gw)
    with pytest.raises(L.LnxError, match="task_keys"):
        FusedHierarchicalLoss(["taxa_L20"], {"taxa_L20": torch.nn.CrossEntropyLoss(reduction="none")}, gw)
    f = FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": TaxonomyAwareLabelSmoothingCE(torch.eye(3))}, gw)
    sched = NS(get_null_mask_prob=lambda s: 1.0)
    with pytest.raises(L.LnxError, match="CPU tensors"):
        f({"taxa_L10": torch.zeros(2, 3)}, {"taxa_L10": torch.zeros(2, dtype=torch.long)}, sched, 0)
    with pytest.raises(L.LnxError, match="dict-valued"):
        f({"taxa_L10": {"x": torch.zeros(2, 3)}}, {"taxa_L10": torch.zeros(2, dtype=torch.long)}, sched, 0)
