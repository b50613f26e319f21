"""The fused hierarchical loss on the GPU (lnx_hier_loss_fwd / lnx_hier_loss_bwd behind linnaeus_amd.loss.FusedHierarchicalLoss) against
the reference's recorded numbers, against the composed path on the same device tensors, and against the float64 restatement of
tests/test_hier_loss.py.  Tolerances are tests/test_loss.py's: totals and components rtol 2e-5, gradients rtol 2e-4 / atol 2e-6."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from tests.test_hier_loss import MODES, SOFT_MODES, check_against_fixture, fixture_case, hier_ref

pytestmark = pytest.mark.gpu

CFG = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=False), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=True, VAL=False))))


def sched(p):
    return NS(get_null_mask_prob=lambda step: p)


def soft_matrix(c, g):
    m = 0.9 * torch.eye(c) + 0.1 * torch.softmax(torch.randn(c, c, generator=g), 1)
    return m / m.sum(1, keepdim=True)


def make_case(heads, B, seed, *, dtype=torch.float32, kinds=None, class_weights=True, null_rows=3, weighting="static", ignore_index=None, cfg=CFG):
    """seeded logits / hard targets / criteria / GradientWeighting for `heads` = ((task, C), ...); kinds[i] in {"soft", "ce"}"""
    from linnaeus_amd.loss import GradientWeighting, TaxonomyAwareLabelSmoothingCE

    g = torch.Generator().manual_seed(seed)
    tasks = [t for t, _ in heads]
    kinds = kinds or ["soft"] * len(heads)
    base, tg, crit, cw = {}, {}, {}, {}
    for (t, c), kind in zip(heads, kinds):
        base[t] = (torch.randn(B, c, generator=g) * 2).to(dtype).cuda()
        y = torch.randint(0, c, (B,), generator=g)
        y[:min(null_rows, B)] = 0
        tg[t] = y.cuda()
        if kind == "soft":
            crit[t] = TaxonomyAwareLabelSmoothingCE(soft_matrix(c, g), ignore_index=ignore_index).cuda()
            crit[t].validate_targets = False
        else:
            crit[t] = torch.nn.CrossEntropyLoss(reduction="none", label_smoothing=0.1)
        cw[t] = {i: float(0.5 + torch.rand(1, generator=g).item()) for i in range(0, c, 2)}
    tw = {t: float(0.3 + torch.rand(1, generator=g).item()) for t in tasks}
    gw = GradientWeighting(tasks, cfg, weighting, init_weights=tw, class_weights=cw if class_weights else None).cuda()
    return NS(tasks=tasks, base=base, tg=tg, crit=crit, gw=gw, cfg=cfg, B=B)


def run_path(case, fused, prob, *, coin=None, is_validation=False, targets=None, go=None, sync_components=False):
    """one forward + backward through weighted_hierarchical_loss on fresh leaves of the case's logits"""
    from linnaeus_amd.loss import weighted_hierarchical_loss

    lg = {t: case.base[t].clone().requires_grad_(True) for t in case.tasks}
    total, comps, weights = weighted_hierarchical_loss(lg, targets or case.tg, case.crit, case.gw, sched(prob), 0, is_validation=is_validation, config=case.cfg,
                                                       sync_components=sync_components, _coin=coin, fused=fused)
    (total if go is None else total * go).backward()
    return NS(total=total.detach(), comps=comps, weights=weights, grads={t: lg[t].grad for t in case.tasks})


def assert_same_as_composed(f, c, tasks, B):
    np.testing.assert_allclose(float(f.total), float(c.total), rtol=2e-5, atol=0)
    for key in ("weighted_tasks", "tasks", "masked_tasks"):
        np.testing.assert_allclose([float(f.comps[key][t]) for t in tasks], [float(c.comps[key][t]) for t in tasks], rtol=2e-5, atol=0, err_msg=key)
    fs, cs = f.comps["null_masking"], c.comps["null_masking"]
    assert sorted(fs) == sorted(cs)
    for key in ("null_samples_total", "null_samples_included"):
        assert int(fs[key]) == int(cs[key]), key
    np.testing.assert_allclose(float(fs["inclusion_percentage"]), float(cs["inclusion_percentage"]), rtol=2e-5)
    assert fs["null_mask_prob"] == cs["null_mask_prob"] and fs["phase1_active"] == cs["phase1_active"]
    for t in tasks:
        if "num_valid_samples_per_task" in cs:
            assert int(fs["num_valid_samples_per_task"][t]) == int(cs["num_valid_samples_per_task"][t]), t
        gf, gc = f.grads[t].float(), c.grads[t].float()
        assert gf.dtype == gc.dtype and f.grads[t].dtype == c.grads[t].dtype
        assert torch.equal(gf.abs().sum(1) != 0, gc.abs().sum(1) != 0), f"{t}: the kept rows differ"
        # bf16 leaves: both paths round an fp32 gradient to bf16, and two fp32 values a rounding error apart can land on neighbouring
        # bf16 numbers: one bf16 ulp, at most 2^-7 of the value
        rtol = 2e-4 if f.grads[t].dtype == torch.float32 else 2.0 ** -7
        np.testing.assert_allclose(gf.cpu().numpy(), gc.cpu().numpy(), rtol=rtol, atol=2e-6, err_msg=t)
        np.testing.assert_allclose(f.comps["raw_per_sample_losses"][t].cpu().numpy(), c.comps["raw_per_sample_losses"][t].cpu().numpy(), rtol=2e-5, atol=1e-6)
    assert sorted(f.weights) == sorted(c.weights)
    for t in tasks:
        assert float(f.weights[t]) == pytest.approx(float(c.weights[t]))


# ------------------------------------------------------------------------------------------------------------------ reference fixtures
@pytest.mark.parametrize("name,mode", [("hier_loss.npz", m) for m in MODES] + [("hier_loss_soft.npz", m) for m in SOFT_MODES])
def test_fused_matches_the_reference(name, mode):
    from linnaeus_amd.loss import GradientWeighting, TaxonomyAwareLabelSmoothingCE, weighted_hierarchical_loss

    z, tasks, cfg, cwd, _, _ = fixture_case(name, mode)
    prob, phase1, val, _ = MODES[mode]
    lg = {t: torch.from_numpy(z[f"logits_{t}"]).cuda().requires_grad_(True) for t in tasks}
    tg = {t: torch.from_numpy(z[f"target_{t}"]).cuda() for t in tasks}
    crit = {t: TaxonomyAwareLabelSmoothingCE(torch.from_numpy(z[f"soft_{t}"])).cuda() for t in tasks}
    tw = {t: float(w) for t, w in zip(tasks, z["task_weights"])}
    gw = GradientWeighting(tasks, cfg, "static", init_weights=tw, class_weights=cwd)
    total, comps, weights = weighted_hierarchical_loss(lg, tg, crit, gw, sched(prob), 10, is_validation=val, config=cfg, fused=True)
    total.backward()
    check_against_fixture(z, tasks, mode, total.item(), [comps["weighted_tasks"][t] for t in tasks], [comps["tasks"][t] for t in tasks],
                          [comps["masked_tasks"][t] for t in tasks], [lg[t].grad.cpu().numpy() for t in tasks])
    assert comps["total"] == total.item() and weights == pytest.approx(tw)
    assert comps["null_masking"]["phase1_active"] == (phase1 and not val)


# ------------------------------------------------------------------------------------------------------------------ the composed path
@pytest.mark.parametrize("soft_targets", [False, True])
def test_fused_matches_composed_with_injected_draws(soft_targets):
    heads = (("taxa_L10", 23), ("taxa_L20", 9), ("taxa_L30", 4))
    case = make_case(heads, 65, 5, null_rows=20)
    g = torch.Generator().manual_seed(6)
    coin = {t: torch.rand(65, generator=g).cuda() for t in case.tasks}
    targets = None
    if soft_targets:  # mixup of the hard labels with a permutation of themselves: null where class 0 keeps more than half
        perm = torch.randperm(65, generator=g).cuda()
        targets = {}
        for t, c in heads:
            one = torch.nn.functional.one_hot(case.tg[t], c).float()
            targets[t] = 0.6 * one + 0.4 * one[perm]
    f = run_path(case, True, 0.5, coin=coin, targets=targets)
    c = run_path(case, False, 0.5, coin=coin, targets=targets)
    assert_same_as_composed(f, c, case.tasks, 65)
    n = f.comps["null_masking"]
    assert 0 < int(n["null_samples_included"]) < int(n["null_samples_total"])


def test_fused_draws_what_the_composed_path_draws():
    """0 < prob < 1 without injected draws: with the same torch seed both paths keep the same rows"""
    case = make_case((("taxa_L10", 7), ("taxa_L20", 5)), 33, 7, null_rows=16)
    torch.manual_seed(11)
    f = run_path(case, True, 0.4)
    torch.manual_seed(11)
    c = run_path(case, False, 0.4)
    assert_same_as_composed(f, c, case.tasks, 33)
    n = f.comps["null_masking"]
    assert 0 < int(n["null_samples_included"]) < int(n["null_samples_total"])


# ------------------------------------------------------------------------------------------------------------------ shapes, through the C ABI
SENTINEL = -12345.0


def run_abi(Cs, B, dtype, pad_value, seed, n_pad=5):
    """lnx_hier_loss_fwd + lnx_hier_loss_bwd on seeded inputs: logits rows of C + n_pad elements whose padding holds `pad_value`, dlogits rows
    of C + 3 elements pre-filled with SENTINEL; odd tasks are plain cross entropy with smoothing 0.1, even ones carry a soft matrix"""
    g = torch.Generator().manual_seed(seed)
    T = len(Cs)
    tdt = torch.bfloat16 if dtype == L.BF16 else torch.float32
    a = L.HierLossArgs()
    counts = torch.zeros(L.HL_COUNTS, dtype=torch.int64).cuda()
    out = torch.full((L.HL_OUT_FLOATS,), float("nan")).cuda()
    ws = torch.full((T, L.HL_WS_ROWS, B), float("nan")).cuda()
    draws = torch.rand(T, B, generator=g).cuda()
    weights = (0.3 + torch.rand(T, generator=g)).cuda()
    a.dtype, a.B, a.n_tasks, a.prob, a.mask_mul = dtype, B, T, 0.5, 0
    a.draws, a.weights, a.ws, a.out, a.counts = draws.data_ptr(), weights.data_ptr(), ws.data_ptr(), out.data_ptr(), counts.data_ptr()
    keep, ref_in = [], dict(logits=[], targets=[], soft=[], smoothing=[], cw=[], p_cw=[], p_w=[], draws=[])
    dls = []
    for i, c in enumerate(Cs):
        x = torch.full((B, c + n_pad), pad_value).to(tdt)
        x[:, :c] = (torch.randn(B, c, generator=g) * 2).to(tdt)
        y = torch.randint(0, c, (B,), generator=g)
        y[::3] = 0
        soft = soft_matrix(c, g) if i % 2 == 0 else None
        cw = 0.5 + torch.rand(c, generator=g)
        dl = torch.full((B, c + 3), SENTINEL)
        dev = [v.cuda() if v is not None else None for v in (x, y, soft, cw, dl)]
        k = a.task[i]
        k.logits, k.ld, k.C, k.target = dev[0].data_ptr(), c + n_pad, c, dev[1].data_ptr()
        k.soft, k.smoothing, k.ignore_index = (dev[2].data_ptr() if soft is not None else None), (0.0 if soft is not None else 0.1), -1
        k.class_weight, k.n_cw, k.p_cw, k.p_w = dev[3].data_ptr(), c, i % 3, i % 3 + 1
        k.dlogits, k.ldd = dev[4].data_ptr(), c + 3
        keep.append(dev)
        dls.append(dev[4])
        ref_in["logits"].append(x[:, :c].float().numpy()), ref_in["targets"].append(y.numpy()), ref_in["soft"].append(None if soft is None else soft.numpy())
        ref_in["smoothing"].append(0.1), ref_in["cw"].append(cw.numpy()), ref_in["p_cw"].append(i % 3), ref_in["p_w"].append(i % 3 + 1)
        ref_in["draws"].append(draws[i].cpu().numpy())
    go = torch.tensor([1.0]).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().lnx_hier_loss_fwd(C.byref(a), st), "lnx_hier_loss_fwd")
    L.check(L.lib().lnx_hier_loss_bwd(C.byref(a), C.c_void_p(go.data_ptr()), st), "lnx_hier_loss_bwd")
    torch.cuda.synchronize()
    return NS(out=out.cpu(), counts=counts.cpu(), ws=ws.cpu(), dl=[d.cpu() for d in dls], weights=weights.cpu().numpy(), ref_in=ref_in)


@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("Cs", [(1000,), (2, 63, 64, 65, 256, 257, 1000, 2)], ids=["1task", "8tasks"])
def test_shapes_padding_and_sentinel(Cs, B, dtype):
    r = run_abi(Cs, B, dtype, float("nan"), 100 + B)
    clean = run_abi(Cs, B, dtype, 0.0, 100 + B)
    T, M = len(Cs), L.METRICS_MAX_TASKS
    # NaN in the padding columns of the logits changes no bit of any output
    used = [j * M + t for j in range(4) for t in range(T)] + [L.HL_OUT_TOTAL, L.HL_OUT_INCLUSION]
    assert torch.isfinite(r.out[used]).all() and torch.isfinite(r.ws[:, :L.HL_WS_FLAGS]).all()
    assert torch.equal(r.out[used], clean.out[used]) and torch.equal(r.counts, clean.counts)
    assert torch.equal(r.ws.view(torch.int32), clean.ws.view(torch.int32))
    q = r.ref_in
    ref = hier_ref(q["logits"], q["targets"], q["soft"], r.weights, 0.5, smoothing=q["smoothing"], cw=q["cw"], p_cw=q["p_cw"], p_w=q["p_w"], draws=q["draws"])
    for t, c in enumerate(Cs):
        d = r.dl[t]
        assert torch.equal(d, clean.dl[t])
        assert (d[:, c:] == SENTINEL).all(), f"task {t}: a column >= C was written"
        assert (d[:, :c] != SENTINEL).all() and torch.isfinite(d[:, :c]).all(), f"task {t}: a row was not written"
        np.testing.assert_allclose(d[:, :c].numpy(), ref["grads"][t], rtol=2e-4, atol=2e-6, err_msg=f"task {t}")
        flags = r.ws[t, L.HL_WS_FLAGS].view(torch.int32).numpy()
        assert np.array_equal(flags & 2 != 0, ref["keep"][t]) and np.array_equal(flags & 1 != 0, ref["null"][t])
        assert int(r.counts[t]) == ref["nvalid"][t]
        np.testing.assert_allclose(r.ws[t, L.HL_WS_RAW].numpy(), ref["raw"][t], rtol=2e-5)
    for j, key in ((L.HL_OUT_RAW_MEAN, "raw_mean"), (L.HL_OUT_MASKED_MEAN, "masked_mean"), (L.HL_OUT_WEIGHTED, "weighted"), (L.HL_OUT_SCALE, "scale")):
        np.testing.assert_allclose(r.out[j * M:j * M + T].numpy(), ref[key], rtol=2e-5, err_msg=key)
    np.testing.assert_allclose(float(r.out[L.HL_OUT_TOTAL]), ref["total"], rtol=2e-5)
    np.testing.assert_allclose(float(r.out[L.HL_OUT_INCLUSION]), ref["inclusion_percentage"], rtol=2e-5)
    assert int(r.counts[L.HL_NULL_TOTAL]) == ref["null_total"] and int(r.counts[L.HL_NULL_INCLUDED]) == ref["null_included"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_padded_views_through_python(dtype):
    """logits as column slices of wider buffers (what the model's plan hands out), eight tasks, both storage types, against the composed path"""
    heads = tuple((f"taxa_L{10 * (i + 1)}", c) for i, c in enumerate((2, 63, 64, 65, 256, 257, 1000, 5)))
    # (torch's own cross entropy, the composed path's plain-CE criterion, computes bf16 logits in bf16: no yardstick there)
    case = make_case(heads, 65, 9, dtype=dtype, kinds=["soft", "ce"] * 4 if dtype == torch.float32 else ["soft"] * 8)
    for t, c in heads:
        wide = torch.full((65, c + 5), float("nan"), dtype=dtype).cuda()
        wide[:, :c] = case.base[t]
        case.base[t] = wide[:, :c]
    from linnaeus_amd.loss import weighted_hierarchical_loss

    res = {}
    for fused in (True, False):
        lg = {t: case.base[t].detach().requires_grad_(True) for t in case.tasks}  # leaves that keep the padded pitch
        assert all(v.stride(0) == v.shape[1] + 5 for v in lg.values())
        total, comps, weights = weighted_hierarchical_loss(lg, case.tg, case.crit, case.gw, sched(1.0), 0, config=case.cfg, sync_components=False, fused=fused)
        total.backward()
        res[fused] = NS(total=total.detach(), comps=comps, weights=weights, grads={t: lg[t].grad for t in case.tasks})
    assert_same_as_composed(res[True], res[False], case.tasks, 65)


# ------------------------------------------------------------------------------------------------------------------ edge semantics
def test_all_null_task_with_prob_zero():
    case = make_case((("taxa_L10", 7), ("taxa_L20", 5)), 9, 21)
    case.tg["taxa_L20"] = torch.zeros(9, dtype=torch.long).cuda()
    f, c = run_path(case, True, 0.0), run_path(case, False, 0.0)
    assert_same_as_composed(f, c, case.tasks, 9)
    assert int(f.comps["null_masking"]["num_valid_samples_per_task"]["taxa_L20"]) == 0
    assert float(f.comps["weighted_tasks"]["taxa_L20"]) == 0.0 and not f.grads["taxa_L20"].any()
    assert torch.isfinite(f.total) and all(torch.isfinite(g).all() for g in f.grads.values())


def test_kept_row_with_zero_loss_is_not_counted():
    from linnaeus_amd.loss import TaxonomyAwareLabelSmoothingCE

    case = make_case((("taxa_L10", 6),), 8, 22, class_weights=False, null_rows=0)
    case.crit["taxa_L10"] = TaxonomyAwareLabelSmoothingCE(torch.eye(6)).cuda()
    case.crit["taxa_L10"].validate_targets = False
    case.tg["taxa_L10"] = torch.tensor([1, 2, 3, 4, 5, 1, 2, 3]).cuda()
    sat = torch.full((6,), -100.0)
    sat[2] = 100.0
    case.base["taxa_L10"][1] = sat.cuda()  # row 1, target 2: log-sum-exp == its own logit, the loss is exactly 0.0
    f, c = run_path(case, True, 1.0), run_path(case, False, 1.0)
    assert float(f.comps["raw_per_sample_losses"]["taxa_L10"][1]) == 0.0
    assert int(f.comps["null_masking"]["num_valid_samples_per_task"]["taxa_L10"]) == 7
    assert_same_as_composed(f, c, case.tasks, 8)


def test_criterion_with_ignore_index():
    case = make_case((("taxa_L10", 7), ("taxa_L20", 5)), 12, 23, ignore_index=3)
    case.tg["taxa_L10"][4:7] = 3
    case.tg["taxa_L20"][5:9] = 3
    f, c = run_path(case, True, 0.0), run_path(case, False, 0.0)
    assert_same_as_composed(f, c, case.tasks, 12)
    assert not f.grads["taxa_L10"][4:7].any() and int(f.comps["null_masking"]["num_valid_samples_per_task"]["taxa_L10"]) <= 12 - 3 - 3


def test_plain_cross_entropy_mixed_with_soft_matrix_tasks():
    heads = (("taxa_L10", 11), ("taxa_L20", 6), ("taxa_L30", 4), ("taxa_L40", 3))
    case = make_case(heads, 17, 24, kinds=["ce", "soft", "ce", "soft"])
    coin = {t: torch.rand(17, generator=torch.Generator().manual_seed(i)).cuda() for i, t in enumerate(case.tasks)}
    assert_same_as_composed(run_path(case, True, 0.5, coin=coin), run_path(case, False, 0.5, coin=coin), case.tasks, 17)
    assert_same_as_composed(run_path(case, True, 0.0, is_validation=True), run_path(case, False, 0.0, is_validation=True), case.tasks, 17)


def test_phase1_branch_matches_composed():
    cfg = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=True), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=False, VAL=True))))
    case = make_case((("taxa_L10", 7), ("taxa_L20", 5)), 10, 25, cfg=cfg)
    assert_same_as_composed(run_path(case, True, 1.0), run_path(case, False, 1.0), case.tasks, 10)
    assert_same_as_composed(run_path(case, True, 1.0, is_validation=True), run_path(case, False, 1.0, is_validation=True), case.tasks, 10)


# ------------------------------------------------------------------------------------------------------------------ autograd, weights, determinism
def test_upstream_gradient_scales_exactly():
    case = make_case((("taxa_L10", 23), ("taxa_L20", 9)), 16, 31)
    one = run_path(case, True, 0.0)
    s = torch.tensor(1024.0).cuda()  # what GradScaler multiplies the loss by: a device scalar, never read on the host
    big = run_path(case, True, 0.0, go=s)
    for t in case.tasks:
        assert one.grads[t].any() and torch.equal(big.grads[t], one.grads[t] * 1024.0), t


def test_gradnorm_weights_are_read_on_the_device_without_a_sync():
    from linnaeus_amd.loss import FusedHierarchicalLoss

    heads = (("taxa_L10", 23), ("taxa_L20", 9), ("taxa_L30", 4))
    case = make_case(heads, 16, 32, weighting="gradnorm")
    static = make_case(heads, 16, 32)
    new_w = torch.tensor([2.0, 0.25, 1.5]).cuda()
    coin = {t: torch.rand(16, generator=torch.Generator().manual_seed(i)).cuda() for i, t in enumerate(case.tasks)}
    fused = FusedHierarchicalLoss(case.tasks, case.crit, case.gw, case.cfg)
    fused_static = FusedHierarchicalLoss(static.tasks, static.crit, static.gw, static.cfg)
    lg = [{t: case.base[t].clone().requires_grad_(True) for t in case.tasks} for _ in range(3)]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t1, c1, w1 = fused(lg[0], case.tg, sched(0.5), 0, _coin=coin)
        t1.backward()
        w1 = {t: w.clone() for t, w in w1.items()}
        case.gw.gradnorm.task_weights.copy_(new_w)  # what lnx_gradnorm_update does between two steps
        t2, c2, w2 = fused(lg[1], case.tg, sched(0.5), 1, _coin=coin)
        t2.backward()
        t3, c3, w3 = fused_static(lg[2], static.tg, sched(0.5), 2, _coin=coin)  # static weights, training, sync_components=False
        t3.backward()
        t1, t2, t3 = t1.detach(), t2.detach(), t3.detach()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    old_w = static.gw.task_weights  # the gradnorm case was built from the same seed: these were its initial weights
    raw = {t: float(c1["weighted_tasks"][t]) / float(old_w[i]) for i, t in enumerate(case.tasks)}
    for i, t in enumerate(case.tasks):
        assert float(w1[t]) == pytest.approx(float(old_w[i])) and float(w2[t]) == float(new_w[i])
        assert float(c2["weighted_tasks"][t]) == pytest.approx(raw[t] * float(new_w[i]), rel=1e-6)
        np.testing.assert_allclose(lg[1][t].grad.cpu().numpy(), (lg[0][t].grad * (new_w[i] / old_w[i])).cpu().numpy(), rtol=1e-5, atol=1e-9)
    assert float(t2) == pytest.approx(sum(raw[t] * float(new_w[i]) for i, t in enumerate(case.tasks)), rel=1e-6)
    assert float(t3) == pytest.approx(float(t1), rel=1e-6) and isinstance(c3["total"], torch.Tensor) and isinstance(w3["taxa_L10"], float)
    # and the composed path agrees with the overwritten weights
    assert_same_as_composed(run_path(case, True, 0.5, coin=coin), run_path(case, False, 0.5, coin=coin), case.tasks, 16)


def test_two_calls_give_the_same_bits_and_no_grad_allocates_no_gradient():
    heads = (("taxa_L10", 1000), ("taxa_L20", 257), ("taxa_L30", 64))
    case = make_case(heads, 65, 33, null_rows=20)
    coin = {t: torch.rand(65, generator=torch.Generator().manual_seed(i)).cuda() for i, t in enumerate(case.tasks)}
    a, b = run_path(case, True, 0.5, coin=coin), run_path(case, True, 0.5, coin=coin)
    assert torch.equal(a.total, b.total)
    for key in ("weighted_tasks", "tasks", "masked_tasks", "raw_per_sample_losses"):
        for t in case.tasks:
            assert torch.equal(a.comps[key][t], b.comps[key][t]), (key, t)
    for t in case.tasks:
        assert torch.equal(a.grads[t], b.grads[t]), t
        assert a.grads[t].data_ptr() != b.grads[t].data_ptr()
    from linnaeus_amd.loss import weighted_hierarchical_loss

    with torch.no_grad():
        total, comps, _ = weighted_hierarchical_loss({t: case.base[t].clone().requires_grad_(True) for t in case.tasks}, case.tg, case.crit, case.gw,
                                                     sched(0.5), 0, config=case.cfg, sync_components=True, _coin=coin, fused=True)
    assert total.grad_fn is None and not total.requires_grad and torch.equal(total, a.total)
    assert isinstance(comps["total"], float) and comps["total"] == float(a.total)
    assert comps["weighted_tasks"]["taxa_L20"] == float(a.comps["weighted_tasks"]["taxa_L20"])


def test_mixed_logits_dtypes_are_refused():
    case = make_case((("taxa_L10", 7), ("taxa_L20", 5)), 4, 34)
    case.base["taxa_L20"] = case.base["taxa_L20"].bfloat16()
    with pytest.raises(L.LnxError, match="taxa_L20"):
        run_path(case, True, 1.0)


# ------------------------------------------------------------------------------------------------------------------ through the model
def test_training_step_through_the_model():
    """tiny_a, B = 16, fp32: one step with fused=True and one with fused=False from the same state -- the same loss within rtol 2e-5,
    every parameter gradient within the fp32 bound of tests/test_gpu_model.py (per parameter 2e-3 of max(its norm, 1e-3))"""
    from linnaeus_amd import build_model
    from linnaeus_amd.loss import GradientWeighting, TaxonomyAwareLabelSmoothingCE, weighted_hierarchical_loss
    from oracle import mformer_oracle as O
    from tests.cases import CASES, SEED, make_config

    spec = CASES["tiny_a"]
    sd = O.seeded_state_dict(O.param_shapes(spec), SEED)
    x, meta = O.seeded_inputs(spec, 16, 64, SEED + 1)
    g = torch.Generator().manual_seed(41)
    tasks = [t for t, _ in spec.heads]
    tg, crit, cw = {}, {}, {}
    for t, c in spec.heads:
        y = torch.randint(0, c, (16,), generator=g)
        y[:5] = 0
        tg[t] = y.cuda()
        crit[t] = TaxonomyAwareLabelSmoothingCE(soft_matrix(c, g)).cuda()
        crit[t].validate_targets = False
        cw[t] = {i: float(0.5 + torch.rand(1, generator=g).item()) for i in range(0, c, 2)}
    coin = {t: torch.rand(16, generator=g).cuda() for t in tasks}
    gw = GradientWeighting(tasks, CFG, "static", init_weights={"taxa_L10": 1.0, "taxa_L20": 0.5}, class_weights=cw)
    got = {}
    for fused in (True, False):
        model = build_model(make_config(spec, 64), num_classes={t: c for t, c in spec.heads})
        model.load_state_dict(sd, strict=True)
        model = model.cuda().train()
        model.set_compute_dtype("fp32")
        out = model(x.cuda(), meta.cuda())
        loss, _, _ = weighted_hierarchical_loss(out, tg, crit, gw, sched(0.5), 0, config=CFG, sync_components=False, _coin=coin, fused=fused)
        loss.backward()
        got[fused] = (float(loss), {k: p.grad.float().cpu() for k, p in model.named_parameters()})
    assert abs(got[True][0] - got[False][0]) <= 2e-5 * abs(got[False][0]), (got[True][0], got[False][0])
    assert sorted(got[True][1]) == sorted(got[False][1])
    for k, ref in got[False][1].items():
        err, denom = (got[True][1][k] - ref).norm().item(), ref.norm().item()
        assert err <= 2e-3 * max(denom, 1e-3), (k, err, denom)
    assert sum(v.norm().item() for v in got[False][1].values()) > 0
