"""CrossEntropyLoss, LabelSmoothingCrossEntropy and SoftTargetCrossEntropy on the GPU (lnx_softce with the off-target and soft-row
forms) and inside the fused hierarchical loss (lnx_hier_loss_fwd / _bwd): against the reference's recorded numbers in
tests/golden/basic_loss.npz, against the composed path on the same device tensors, and against the float64 restatement of
tests/basic_loss_ref.py.  Tolerances are tests/test_loss.py's: losses and components rtol 2e-5 / atol 2e-6, gradients rtol 2e-4 /
atol 2e-6; a gradient stored as bf16 is one more rounding, at most 2^-7 of the value (tests/test_gpu_hier_loss.py)."""
import ctypes as C
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from tests.basic_loss_ref import basic_ref
from tests.test_basic_loss import CASES, GOLDEN, HIER_MODES
from tests.test_gpu_hier_loss import CFG, assert_same_as_composed, run_path, sched, soft_matrix
from tests.test_hier_loss import MODES, check_against_fixture

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def criterion(kind, weight=None, ignore_index=None, smoothing=0.0, validate=False):
    from linnaeus_amd.loss import CrossEntropyLoss, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy

    apply_w = weight is not None
    if kind == "ce":
        crit = CrossEntropyLoss(weight, apply_w, ignore_index)
    elif kind == "ls":
        crit = LabelSmoothingCrossEntropy(weight, smoothing, apply_w, ignore_index)
    else:
        crit = SoftTargetCrossEntropy(weight, apply_w)
    crit.validate_targets = validate
    return crit


def run_class(crit, x, y, go=None):
    leaf = x.clone().requires_grad_(True)
    loss = crit(leaf, y)
    assert loss.shape == (x.shape[0],) and loss.dtype == torch.float32
    (loss if go is None else loss * go).sum().backward()
    return loss.detach(), leaf.grad


# ------------------------------------------------------------------------------------------------------------------ the reference's numbers
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_classes_match_the_reference(golden, case):
    key, kind, c, tname, wi, ign, eps = case
    w = torch.from_numpy(golden[f"weight_C{c}"]) if wi else None  # a CPU tensor, as the reference's builder leaves it
    crit = criterion(kind, w, ign, eps, validate=True)
    loss, grad = run_class(crit, torch.from_numpy(golden[f"logits_C{c}"]).cuda(), torch.from_numpy(golden[tname]).cuda(), torch.from_numpy(golden[f"go_C{c}"]).cuda())
    np.testing.assert_allclose(loss.cpu().numpy(), golden[key + "_loss"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(grad.cpu().numpy(), golden[key + "_grad"], rtol=2e-4, atol=2e-6)


def hier_fixture_case(z, mode, dtype=torch.float32):
    from linnaeus_amd.loss import GradientWeighting

    prob, phase1, val, _ = MODES[mode]
    tasks = [str(t) for t in z["tasks"]]
    cfg = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=phase1), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=True, VAL=False))))
    base, tg, crit, cwd = {}, {}, {}, {}
    for t, c, kind in zip(tasks, z["hier_classes"], z["hier_kinds"]):
        c, kind = int(c), str(kind)
        base[t] = torch.from_numpy(z[f"logits_C{c}"]).to(dtype).cuda()
        tg[t] = torch.from_numpy(z[{"ce": "hard", "ls": "rows", "st": "strows"}[kind] + f"_C{c}"]).cuda()
        crit[t] = criterion(kind, torch.from_numpy(z[f"weight_C{c}"]), 0 if (phase1 and kind != "st") else None, 0.1)
        cwd[t] = {i: float(z[f"cw_{t}"][i]) for i in range(0, c, 2)}
    tw = {t: float(w) for t, w in zip(tasks, z["task_weights"])}
    gw = GradientWeighting(tasks, cfg, "static", init_weights=tw, class_weights=cwd)
    return NS(tasks=tasks, base=base, tg=tg, crit=crit, gw=gw, cfg=cfg, B=16), prob, val


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("mode", HIER_MODES)
def test_hierarchical_loss_matches_the_reference(golden, mode, fused):
    case, prob, val = hier_fixture_case(golden, mode)
    r = run_path(case, fused, prob, is_validation=val, sync_components=True)
    check_against_fixture(golden, case.tasks, mode, float(r.total), [r.comps["weighted_tasks"][t] for t in case.tasks], [r.comps["tasks"][t] for t in case.tasks],
                          [r.comps["masked_tasks"][t] for t in case.tasks], [r.grads[t].cpu().numpy() for t in case.tasks])


# ------------------------------------------------------------------------------------------------------------------ the composed path
HEADS8 = tuple((f"taxa_L{10 * (i + 1)}", c) for i, c in enumerate((2, 3, 255, 256, 257, 1000, 5, 9)))
KINDS8 = ("st", "ls", "ce", "soft", "torch", "st", "ls", "ce")  # all five forms of the row in one call


def mixes(y, c, g, lam=0.6):
    """[B, C] mixup rows of the hard labels with a permutation of themselves: null where class 0 keeps more than half"""
    one = torch.nn.functional.one_hot(y, c).float()
    return lam * one + (1.0 - lam) * one[torch.randperm(y.shape[0], generator=g)]


def make_case8(B, seed, dtype=torch.float32, cfg=CFG):
    from linnaeus_amd.loss import GradientWeighting, TaxonomyAwareLabelSmoothingCE

    g = torch.Generator().manual_seed(seed)
    tasks = [t for t, _ in HEADS8]
    base, tg, crit, cw = {}, {}, {}, {}
    for i, ((t, c), kind) in enumerate(zip(HEADS8, KINDS8)):
        base[t] = (torch.randn(B, c, generator=g) * 2).to(dtype).cuda()
        y = torch.randint(0, c, (B,), generator=g)
        y[:min(5, B)] = 0
        w = 0.5 + torch.rand(c, generator=g)
        if kind == "soft":
            crit[t] = TaxonomyAwareLabelSmoothingCE(soft_matrix(c, g)).cuda()
            crit[t].validate_targets = False
        elif kind == "torch":
            crit[t] = torch.nn.CrossEntropyLoss(reduction="none", label_smoothing=0.1)
            if dtype != torch.float32:  # (torch's own cross entropy computes bf16 logits in bf16: no yardstick there)
                crit[t] = criterion("ce")
        else:  # the first of each kind without a weight, the second with one (and an ignore_index where the kind has one)
            crit[t] = criterion(kind, w if i >= 5 else None, 3 if (i >= 5 and kind != "st") else None, 0.1)
        two_d = kind == "st" or (kind in ("ls", "ce") and i < 5)  # [B, C] targets for every SoftTargetCrossEntropy and for one of each other kind
        tg[t] = (mixes(y, c, g) if two_d else y).cuda()
        cw[t] = {j: float(0.5 + torch.rand(1, generator=g).item()) for j in range(0, c, 2)}
    tw = {t: float(0.3 + torch.rand(1, generator=g).item()) for t in tasks}
    gw = GradientWeighting(tasks, cfg, "static", init_weights=tw, class_weights=cw).cuda()
    return NS(tasks=tasks, base=base, tg=tg, crit=crit, gw=gw, cfg=cfg, B=B)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_eight_tasks_of_all_forms_match_composed_with_injected_draws(dtype):
    case = make_case8(33, 51, dtype)
    coin = {t: torch.rand(33, generator=torch.Generator().manual_seed(i)).cuda() for i, t in enumerate(case.tasks)}
    f, c = run_path(case, True, 0.5, coin=coin), run_path(case, False, 0.5, coin=coin)
    assert_same_as_composed(f, c, case.tasks, 33)
    n = f.comps["null_masking"]
    assert 0 < int(n["null_samples_included"]) < int(n["null_samples_total"])
    assert all(f.grads[t].any() for t in case.tasks)
    assert_same_as_composed(run_path(case, True, 0.0, is_validation=True), run_path(case, False, 0.0, is_validation=True), case.tasks, 33)


def test_phase1_branch_with_ignore_index_matches_composed():
    cfg = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=True), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=False, VAL=True))))
    case = make_case8(16, 52, cfg=cfg)
    for t, kind in zip(case.tasks, KINDS8):
        if kind in ("ce", "ls"):
            case.crit[t].ignore_index = 0  # what prepare_loss_functions builds under PHASE1_MASK_NULL_LOSS
    assert_same_as_composed(run_path(case, True, 1.0), run_path(case, False, 1.0), case.tasks, 16)


# ------------------------------------------------------------------------------------------------------------------ seams, through the C ABI
def padded(rows, pad, fill=float("nan")):
    """`rows` [B, C] as the first C columns of a [B, C + pad] device buffer whose other columns hold `fill`"""
    wide = torch.full((rows.shape[0], rows.shape[1] + pad), fill, dtype=rows.dtype)
    wide[:, :rows.shape[1]] = rows
    return wide.cuda()


def seam_inputs(B, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, c, generator=g) * 2
    y = torch.randint(0, c, (B,), generator=g)
    y[0] = 0
    rows = mixes(y, c, g, 0.7) * (0.8 + 0.4 * torch.rand(B, 1, generator=g))  # sums in [0.8, 1.2]
    return x, y, rows, 0.5 + torch.rand(c, generator=g), 0.5 + torch.rand(B, generator=g)


def softce_abi(form, x, y, rows, w, go, *, ignore_index=-1, smoothing=0.0):
    """one lnx_softce call: logits pitch C + 3, target rows pitch C + 5, NaN in every padding column of both; dlogits pitch C + 3 over SENTINEL"""
    B, c = x.shape
    xd, rd = padded(x, 3), (padded(rows, 5) if form == L.CE_FORM_SOFT_ROW else None)
    yd, wd, god = y.cuda(), w.cuda(), go.cuda()
    loss = torch.full((B,), SENTINEL).cuda()
    dl = torch.full((B, c + 3), SENTINEL).cuda()
    a = L.SoftCEArgs()
    a.B, a.C, a.logits, a.ld = B, c, xd.data_ptr(), c + 3
    a.target = None if form == L.CE_FORM_SOFT_ROW else yd.data_ptr()
    a.smoothing, a.class_weight, a.ignore_index, a.row_scale, a.scale = smoothing, wd.data_ptr(), ignore_index, god.data_ptr(), 1.0
    a.loss, a.dlogits, a.ldd, a.form = loss.data_ptr(), dl.data_ptr(), c + 3, form
    if rd is not None:
        a.soft_target, a.ldt = rd.data_ptr(), c + 5
    L.check(L.lib().lnx_softce(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_softce")
    torch.cuda.synchronize()
    return loss.cpu(), dl.cpu()


@pytest.mark.parametrize("B", [1, 5, 16])
@pytest.mark.parametrize("c", [2, 3, 255, 256, 257, 1000])
def test_row_kernel_seams_padding_and_sentinel(c, B):
    x, y, rows, w, go = seam_inputs(B, c, 1000 * B + c)
    for kind, form, kw in (("ce", L.CE_FORM_DEFAULT, dict(ignore_index=0)), ("ls", L.CE_FORM_OFF_TARGET, dict(ignore_index=0, smoothing=0.1)), ("st", L.CE_FORM_SOFT_ROW, {})):
        loss, dl = softce_abi(form, x, y, rows, w, go, **kw)
        ref_loss, ref_grad = basic_ref(kind, x, rows if kind == "st" else y, w, kw.get("ignore_index"), kw.get("smoothing", 0.0), go)
        assert (dl[:, c:] == SENTINEL).all(), f"{kind}: a column >= C of dlogits was written"
        assert torch.isfinite(loss).all() and torch.isfinite(dl[:, :c]).all(), f"{kind}: a padding column was read"
        np.testing.assert_allclose(loss.numpy(), ref_loss.numpy(), rtol=2e-5, atol=2e-6, err_msg=kind)
        np.testing.assert_allclose(dl[:, :c].numpy(), ref_grad.numpy(), rtol=2e-4, atol=2e-6, err_msg=kind)
        if kind != "st":
            assert loss[0] == 0 and not dl[0, :c].any()  # the ignored row


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B", [1, 5, 16])
@pytest.mark.parametrize("c", [2, 3, 255, 256, 257, 1000])
def test_fused_kernel_seams_padding_and_sentinel(c, B, dtype):
    """lnx_hier_loss_fwd / _bwd, three tasks of the same width (CrossEntropyLoss with ignore_index on [B] targets, LabelSmoothingCrossEntropy and
    SoftTargetCrossEntropy on [B, C] rows), every row kept, unit task weights: dlogits = go / nvalid * the restatement's gradient"""
    x, y, rows, w, _ = seam_inputs(B, c, 2000 * B + c)
    x = x.to(dtype)
    y[B // 2] = min(1, c - 1)  # a row that is neither ignored nor null, so that nvalid > 0 in every task
    rows[B // 2] = torch.nn.functional.one_hot(y[B // 2], c).float() * 0.9
    xd, rd, yd, wd = padded(x, 3), padded(rows, 5), y.cuda(), w.cuda()
    T = 3
    counts = torch.zeros(L.HL_COUNTS, dtype=torch.int64).cuda()
    out = torch.full((L.HL_OUT_FLOATS,), float("nan")).cuda()
    ws = torch.full((T, L.HL_WS_ROWS, B), float("nan")).cuda()
    weights, go = torch.ones(T).cuda(), torch.tensor([0.5]).cuda()
    dls = [torch.full((B, c + 3), SENTINEL).cuda() for _ in range(T)]
    a = L.HierLossArgs()
    a.dtype, a.B, a.n_tasks, a.prob, a.mask_mul = (L.BF16 if dtype == torch.bfloat16 else L.F32), B, T, 1.0, 0
    a.weights, a.ws, a.out, a.counts = weights.data_ptr(), ws.data_ptr(), out.data_ptr(), counts.data_ptr()
    spec = (("ce", L.CE_FORM_DEFAULT, 0, 0.0, y), ("ls", L.CE_FORM_OFF_TARGET, -1, 0.1, rows), ("st", L.CE_FORM_SOFT_ROW, -1, 0.0, rows))
    for i, (kind, form, ign, eps, tgt) in enumerate(spec):
        k = a.task[i]
        k.logits, k.ld, k.C, k.form, k.smoothing, k.crit_weight, k.ignore_index = xd.data_ptr(), c + 3, c, form, eps, wd.data_ptr(), ign
        if tgt is y:
            k.target = yd.data_ptr()
        else:
            k.soft_target, k.ldt = rd.data_ptr(), c + 5
        k.dlogits, k.ldd = dls[i].data_ptr(), c + 3
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.lib().lnx_hier_loss_fwd(C.byref(a), st), "lnx_hier_loss_fwd")
    L.check(L.lib().lnx_hier_loss_bwd(C.byref(a), C.c_void_p(go.data_ptr()), st), "lnx_hier_loss_bwd")
    torch.cuda.synchronize()
    total = 0.0
    for i, (kind, form, ign, eps, tgt) in enumerate(spec):
        ref_loss, ref_grad = basic_ref(kind, x.float(), tgt, w, ign if ign >= 0 else None, eps)
        nvalid = int((ref_loss != 0).sum())
        assert nvalid > 0 and int(counts[i]) == nvalid, kind
        d = dls[i].cpu()
        assert (d[:, c:] == SENTINEL).all(), f"{kind}: a column >= C of dlogits was written"
        assert torch.isfinite(d[:, :c]).all() and torch.isfinite(ws[i, :L.HL_WS_FLAGS]).all(), f"{kind}: a padding column was read"
        np.testing.assert_allclose(ws[i, L.HL_WS_RAW].cpu().numpy(), ref_loss.numpy(), rtol=2e-5, atol=2e-6, err_msg=kind)
        np.testing.assert_allclose(d[:, :c].numpy(), (0.5 / nvalid * ref_grad).numpy(), rtol=2e-4, atol=2e-6, err_msg=kind)
        flags = ws[i, L.HL_WS_FLAGS].cpu().view(torch.int32)
        assert torch.equal(flags >> 3, (tgt if tgt is y else tgt.argmax(1)).to(torch.int32)), f"{kind}: the class kept in the flags"
        assert torch.equal((flags & 1) != 0, (y == 0) if tgt is y else (rows[:, 0] > 0.5)), f"{kind}: the null flag"
        total += float(ref_loss.sum()) / nvalid
    np.testing.assert_allclose(float(out[L.HL_OUT_TOTAL]), total, rtol=2e-5)


def test_bf16_logits_through_the_classes():
    """bf16 logits are widened to fp32 for the launch; the gradient comes back in bf16: one rounding of the fp32 value"""
    x, y, rows, w, go = seam_inputs(16, 257, 77)
    xb = x.bfloat16()
    for kind, tgt in (("ce", y), ("ls", rows), ("st", rows)):
        loss, grad = run_class(criterion(kind, w, None, 0.1), xb.cuda(), tgt.cuda(), go.cuda())
        ref_loss, ref_grad = basic_ref(kind, xb.float(), tgt, w, None, 0.1, go)
        assert grad.dtype == torch.bfloat16
        np.testing.assert_allclose(loss.cpu().numpy(), ref_loss.numpy(), rtol=2e-5, atol=2e-6, err_msg=kind)
        np.testing.assert_allclose(grad.float().cpu().numpy(), ref_grad.numpy(), rtol=2.0 ** -7, atol=2e-6, err_msg=kind)


# ------------------------------------------------------------------------------------------------------------------ exact probes (fp32)
def test_off_target_smoothing_of_zero_is_the_hard_label_form_bit_for_bit():
    x, y, rows, w, go = seam_inputs(16, 257, 78)
    hard = softce_abi(L.CE_FORM_DEFAULT, x, y, rows, w, go, ignore_index=0)
    off = softce_abi(L.CE_FORM_OFF_TARGET, x, y, rows, w, go, ignore_index=0, smoothing=0.0)
    assert torch.equal(hard[0], off[0]) and torch.equal(hard[1], off[1]) and hard[1][:, :257].any()
    # and through the classes, inside the fused loss
    case = make_case8(16, 53)
    fused = {}
    for kind in ("ls", "ce"):
        for t, c in HEADS8:
            case.crit[t] = criterion(kind, None, 3, 0.0)
            case.tg[t] = case.tg[t].argmax(1) if case.tg[t].dim() == 2 else case.tg[t]
        fused[kind] = run_path(case, True, 0.0)
    assert torch.equal(fused["ls"].total, fused["ce"].total)
    for t in case.tasks:
        assert torch.equal(fused["ls"].grads[t], fused["ce"].grads[t]) and fused["ce"].grads[t].any(), t
        assert torch.equal(fused["ls"].comps["raw_per_sample_losses"][t], fused["ce"].comps["raw_per_sample_losses"][t]), t


def test_one_hot_soft_rows_are_the_hard_label_form_bit_for_bit():
    x, y, rows, w, go = seam_inputs(16, 257, 79)
    one = torch.nn.functional.one_hot(y, 257).float()
    hard = softce_abi(L.CE_FORM_DEFAULT, x, y, one, w, go)
    soft = softce_abi(L.CE_FORM_SOFT_ROW, x, y, one, w, go)
    assert torch.equal(hard[0], soft[0]) and torch.equal(hard[1], soft[1]) and hard[1][:, :257].any()
    case = make_case8(16, 54)
    g = torch.Generator().manual_seed(540)
    wts = {t: 0.5 + torch.rand(c, generator=g) for t, c in HEADS8}
    for t, c in HEADS8:  # [B, C] exact one-hot rows for both criteria: CrossEntropyLoss arg-maxes them
        yt = case.tg[t].argmax(1) if case.tg[t].dim() == 2 else case.tg[t]
        case.tg[t] = torch.nn.functional.one_hot(yt, c).float()
    fused = {}
    for kind in ("st", "ce"):
        for t, c in HEADS8:
            case.crit[t] = criterion(kind, wts[t])
        fused[kind] = run_path(case, True, 0.0)
    assert torch.equal(fused["st"].total, fused["ce"].total)
    for t in case.tasks:
        assert torch.equal(fused["st"].grads[t], fused["ce"].grads[t]) and fused["ce"].grads[t].any(), t
        assert torch.equal(fused["st"].comps["raw_per_sample_losses"][t], fused["ce"].comps["raw_per_sample_losses"][t]), t


def test_two_identical_calls_give_the_same_bits():
    x, y, rows, w, go = seam_inputs(16, 1000, 80)
    for kind, tgt in (("ce", y), ("ls", rows), ("st", rows)):
        a = run_class(criterion(kind, w, None, 0.1), x.cuda(), tgt.cuda(), go.cuda())
        b = run_class(criterion(kind, w, None, 0.1), x.cuda(), tgt.cuda(), go.cuda())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[1].any(), kind
    case = make_case8(33, 55)
    coin = {t: torch.rand(33, generator=torch.Generator().manual_seed(i)).cuda() for i, t in enumerate(case.tasks)}
    p, q = run_path(case, True, 0.5, coin=coin), run_path(case, True, 0.5, coin=coin)
    assert torch.equal(p.total, q.total)
    for t in case.tasks:
        assert torch.equal(p.grads[t], q.grads[t]) and torch.equal(p.comps["raw_per_sample_losses"][t], q.comps["raw_per_sample_losses"][t]), t


# ------------------------------------------------------------------------------------------------------------------ fused loss behaviour
def test_upstream_gradient_is_a_device_scalar_and_nothing_is_read_on_the_host():
    from linnaeus_amd.loss import FusedHierarchicalLoss

    case = make_case8(16, 56)
    fused = FusedHierarchicalLoss(case.tasks, case.crit, case.gw, case.cfg)
    lg = [{t: case.base[t].clone().requires_grad_(True) for t in case.tasks} for _ in range(3)]
    coin = {t: torch.rand(16, generator=torch.Generator().manual_seed(i)).cuda() for i, t in enumerate(case.tasks)}
    s = torch.tensor(1024.0).cuda()  # what GradScaler multiplies the loss by
    fused(lg[0], case.tg, sched(0.5), 0, _coin=coin)[0].backward()  # the first call uploads the weight vectors
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t1, c1, _ = fused(lg[1], case.tg, sched(0.5), 1, sync_components=False, _coin=coin)
        t1.backward()
        t2, c2, _ = fused(lg[2], case.tg, sched(0.5), 2, sync_components=False, _coin=coin)
        (t2 * s).backward()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert isinstance(c1["total"], torch.Tensor) and torch.equal(t1.detach(), t2.detach())
    for t in case.tasks:
        assert lg[1][t].grad.any() and torch.equal(lg[2][t].grad, lg[1][t].grad * 1024.0), t
        assert torch.equal(lg[1][t].grad, lg[0][t].grad), t


# ------------------------------------------------------------------------------------------------------------------ failure modes
def test_bad_rows_give_nan_loss_and_a_zero_gradient_row():
    x, y, rows, w, go = seam_inputs(8, 257, 81)
    y[1] = 1
    y[2], y[5] = 257, -100  # past the last class, and torch's own ignore value: only ignore_index is ignored
    for kind in ("ce", "ls"):
        loss, grad = run_class(criterion(kind, w, 0, 0.1), x.cuda(), y.cuda(), go.cuda())
        assert torch.isnan(loss[[2, 5]]).all() and torch.isfinite(loss[[0, 1, 3, 4, 6, 7]]).all(), kind
        assert not grad[[2, 5]].any() and torch.isfinite(grad).all() and grad[1].any(), kind
        ref_loss, ref_grad = basic_ref(kind, x, y, w, 0, 0.1, go)
        np.testing.assert_allclose(grad.cpu().numpy(), ref_grad.numpy(), rtol=2e-4, atol=2e-6)
        with pytest.raises(IndexError, match="2 target indices out of bounds"):  # validate_targets, the default: one host read, then the reference's error
            criterion(kind, w, 0, 0.1, validate=True)(x.cuda(), y.cuda())
    rows[2], rows[5] = float("nan"), float("-inf")
    rows[6, 3] = float("inf")
    loss, grad = run_class(criterion("st", w), x.cuda(), rows.cuda(), go.cuda())
    assert torch.isnan(loss[[2, 5, 6]]).all() and torch.isfinite(loss[[0, 1, 3, 4, 7]]).all()
    assert not grad[[2, 5, 6]].any() and torch.isfinite(grad).all() and grad[1].any()
    # the same rows inside the fused loss: the total is NaN (as the composed path's), the gradient rows are zero and the others finite
    from linnaeus_amd.loss import GradientWeighting

    tasks = ["taxa_L10", "taxa_L20", "taxa_L30"]
    y2 = y.clone()
    y2[5] = 300
    case = NS(tasks=tasks, base={t: x.cuda() for t in tasks}, tg={"taxa_L10": y2.cuda(), "taxa_L20": y2.cuda(), "taxa_L30": rows.cuda()},
              crit={"taxa_L10": criterion("ce", w), "taxa_L20": criterion("ls", w, None, 0.1), "taxa_L30": criterion("st", w)},
              gw=GradientWeighting(tasks, CFG, "static", class_weights={t: {1: 2.0} for t in tasks}), cfg=CFG, B=8)
    f = run_path(case, True, 1.0)
    assert torch.isnan(f.total)
    for t, bad in (("taxa_L10", [2, 5]), ("taxa_L20", [2, 5]), ("taxa_L30", [2, 5, 6])):
        assert torch.isnan(f.comps["raw_per_sample_losses"][t][bad]).all() and not f.grads[t][bad].any() and torch.isfinite(f.grads[t]).all() and f.grads[t][1].any(), t


def test_a_refused_call_launches_nothing():
    from linnaeus_amd.loss import FusedHierarchicalLoss, GradientWeighting

    x = torch.randn(4, 1).cuda()
    loss = torch.full((4,), SENTINEL).cuda()
    dl = torch.full((4, 1), SENTINEL).cuda()
    y = torch.zeros(4, dtype=torch.long).cuda()
    a = L.SoftCEArgs()
    a.B, a.C, a.logits, a.ld, a.target, a.smoothing, a.ignore_index, a.scale = 4, 1, x.data_ptr(), 1, y.data_ptr(), 0.1, -1, 1.0
    a.loss, a.dlogits, a.ldd, a.form = loss.data_ptr(), dl.data_ptr(), 1, L.CE_FORM_OFF_TARGET
    assert L.lib().lnx_softce(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)) != 0
    assert b"C >= 2" in L.lib().lnx_last_error()
    with pytest.raises(L.LnxError, match="C >= 2"):  # LabelSmoothingCrossEntropy on one class: refused by name, not a division by zero
        criterion("ls", None, None, 0.1)(x.requires_grad_(True), y)
    # the fused loss: a weight of the wrong length, a [B] target for SoftTargetCrossEntropy, one class for LabelSmoothingCrossEntropy
    gw = GradientWeighting(["taxa_L10"], CFG, "static")
    lg = {"taxa_L10": torch.randn(4, 3).cuda().requires_grad_(True)}
    y3 = {"taxa_L10": torch.zeros(4, dtype=torch.long).cuda()}
    with pytest.raises(ValueError, match="weight has"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": criterion("ce", torch.ones(2))}, gw, CFG)(lg, y3, sched(1.0), 0)
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": criterion("st")}, gw, CFG)(lg, y3, sched(1.0), 0)
    with pytest.raises(L.LnxError, match="C >= 2"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": criterion("ls", None, None, 0.1)}, gw, CFG)({"taxa_L10": x}, y3, sched(1.0), 0)
    torch.cuda.synchronize()
    assert (loss == SENTINEL).all() and (dl == SENTINEL).all() and lg["taxa_L10"].grad is None
