"""CrossEntropyLoss, LabelSmoothingCrossEntropy and SoftTargetCrossEntropy without a GPU: the plain-torch restatement of
tests/basic_loss_ref.py (the yardstick of tests/test_gpu_basic_loss.py) against the reference's own numbers in tests/golden/basic_loss.npz,
the constructors, the builders and the converter, every new host refusal of lnx_softce / lnx_softce_multi / lnx_hier_loss_fwd / _bwd
(checked before any launch), and the ctypes mirrors of the structs that grew against the C compiler."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from tests.basic_loss_ref import basic_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "basic_loss.npz")
CLASSES = (2, 3, 257)
HIER_MODES = ("sched1", "sched0", "phase1", "val")


def fixture_cases():
    """(key, kind, C, target array name, weighted, ignore_index, smoothing) of every recorded criterion call"""
    out = []
    for c in CLASSES:
        for tk in ("hard", "rows"):
            for wi in (0, 1):
                for ii in (0, 1):
                    out.append((f"ce_C{c}_{tk}_w{wi}_i{ii}", "ce", c, f"{tk}_C{c}", wi, 0 if ii else None, 0.0))
                    for si, eps in enumerate((0.0, 0.1)):
                        out.append((f"ls_C{c}_{tk}_w{wi}_i{ii}_s{si}", "ls", c, f"{tk}_C{c}", wi, 0 if ii else None, eps))
        for wi in (0, 1):
            out.append((f"st_C{c}_rows_w{wi}_i0", "st", c, f"strows_C{c}", wi, None, 0.0))
    return out


CASES = fixture_cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_matches_the_reference(golden, case):
    key, kind, c, tname, wi, ign, eps = case
    loss, grad = basic_ref(kind, golden[f"logits_C{c}"], golden[tname], golden[f"weight_C{c}"] if wi else None, ign, eps, golden[f"go_C{c}"])
    np.testing.assert_allclose(loss.numpy(), golden[key + "_loss"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(grad.numpy(), golden[key + "_grad"], rtol=1e-4, atol=1e-6)


def test_fixture_holds_the_rows_it_is_for(golden):
    assert len(CASES) == 3 * (8 + 16 + 2) and all(k + "_loss" in golden.files and k + "_grad" in golden.files for k, *_ in CASES)
    for c in CLASSES:
        y, rows, st = golden[f"hard_C{c}"], golden[f"rows_C{c}"], golden[f"strows_C{c}"]
        assert y.dtype == np.int64 and y.shape == (16,) and rows.shape == st.shape == (16, c) and rows.dtype == np.float32
        assert 0 < (y == 0).sum() < 16 and 0 < (rows.argmax(1) == 0).sum() < 16  # ignored and kept rows under ignore_index = 0
        assert ((rows == rows.max(1, keepdims=True)).sum(1) == 1).all()  # tie-free maxima
        assert 0 < (rows[:, 0] > 0.5).sum() < 16
        assert ((st > 0).sum(1) == 2).all() and abs(st[5].sum() - 0.8) < 1e-6  # mixes of two classes, one row that sums to 0.8
        np.testing.assert_allclose(np.delete(st.sum(1), 5), 1.0, rtol=1e-6)
        # what ignore_index = 0 means: the recorded loss and gradient rows are exactly zero
        assert (golden[f"ce_C{c}_hard_w1_i1_loss"][y == 0] == 0).all() and (golden[f"ls_C{c}_rows_w0_i1_s1_grad"][rows.argmax(1) == 0] == 0).all()
    assert [str(t) for t in golden["tasks"]] == ["taxa_L10", "taxa_L20", "taxa_L30"] and list(golden["hier_kinds"]) == ["ce", "ls", "st"]
    for mode in HIER_MODES:
        assert np.isfinite(golden[f"{mode}_total"]) and golden[f"{mode}_weighted"].shape == (3,)


def test_restatement_failure_modes():
    x = torch.randn(4, 5, generator=torch.Generator().manual_seed(1))
    for kind in ("ce", "ls"):
        loss, grad = basic_ref(kind, x, torch.tensor([1, 7, -100, 0]), smoothing=0.1)
        assert torch.isnan(loss[1:3]).all() and torch.isfinite(loss[[0, 3]]).all() and not grad[1:3].any() and grad[0].any()
    y = torch.softmax(torch.randn(4, 5, generator=torch.Generator().manual_seed(2)), 1)
    y[1], y[2] = float("nan"), float("-inf")
    loss, grad = basic_ref("st", x, y)
    assert torch.isnan(loss[1:3]).all() and torch.isfinite(loss[[0, 3]]).all() and not grad[1:3].any() and torch.isfinite(grad).all()


# ------------------------------------------------------------------------------------------------------------------ constructors
def test_constructors_and_attributes():
    from linnaeus_amd.loss import CrossEntropyLoss, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy

    w = torch.tensor([1.0, 2.0, 3.0])
    ce = CrossEntropyLoss(w, True, 0)  # positional, in the reference's order
    assert ce.weight is w and ce.apply_class_weights is True and ce.ignore_index == 0 and ce.validate_targets is True
    assert isinstance(ce.criterion, torch.nn.CrossEntropyLoss) and ce.criterion.reduction == "none" and ce.criterion.ignore_index == 0
    ce = CrossEntropyLoss()
    assert ce.weight is None and ce.apply_class_weights is False and ce.ignore_index is None and ce.criterion.ignore_index == -100
    cfg = object()
    ls = LabelSmoothingCrossEntropy(w, 0.2, True, 0, cfg)
    assert ls.weight is w and ls.smoothing == 0.2 and ls.confidence == pytest.approx(0.8) and ls.apply_class_weights is True
    assert ls.ignore_index == 0 and ls.config is cfg and ls.validate_targets is True
    ls = LabelSmoothingCrossEntropy()
    assert ls.smoothing == 0.1 and ls.weight is None and ls.ignore_index is None and ls.config is None
    for bad in (1.0, -0.1):
        with pytest.raises(AssertionError):
            LabelSmoothingCrossEntropy(smoothing=bad)
    st = SoftTargetCrossEntropy(w, True)
    assert st.weight is w and st.apply_class_weights is True and not hasattr(st, "ignore_index")
    assert SoftTargetCrossEntropy().weight is None
    for m in (ce, ls, st):
        assert isinstance(m, torch.nn.Module)


def test_refusals_of_the_classes_need_no_gpu():
    from linnaeus_amd.loss import CrossEntropyLoss, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy

    x = torch.zeros(4, 3)
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        SoftTargetCrossEntropy()(x, torch.zeros(4, dtype=torch.long))  # a [B] target is not broadcast
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        SoftTargetCrossEntropy()(x, torch.zeros(4, 2))
    for crit in (CrossEntropyLoss(), LabelSmoothingCrossEntropy()):
        with pytest.raises(ValueError, match="incompatible"):
            crit(x, torch.zeros(4, 2))
        with pytest.raises(ValueError, match="invalid shape"):
            crit(x, torch.zeros(4, 3, 1))
    # a weight whose length is not C raises at the first call, before anything is launched
    short = torch.ones(2)
    for crit, y in ((CrossEntropyLoss(short, True), torch.zeros(4, dtype=torch.long)), (LabelSmoothingCrossEntropy(short, 0.1, True), torch.zeros(4, dtype=torch.long)),
                    (SoftTargetCrossEntropy(short, True), torch.zeros(4, 3))):
        with pytest.raises(ValueError, match="weight has"):
            crit(x, y)
    # ... and does not apply, so is not looked at, without apply_class_weights; then the missing CPU path is what is reported
    with pytest.raises(L.LnxError, match="no CPU path"):
        CrossEntropyLoss(short, False)(x, torch.zeros(4, dtype=torch.long))


# ------------------------------------------------------------------------------------------------------------------ builders
def make_config(funcs_train, funcs_val, *, cls_train=True, cls_val=False, phase1=False, smoothing=None, tasks=("taxa_L10", "taxa_L20")):
    model = NS() if smoothing is None else NS(LABEL_SMOOTHING=smoothing)
    return NS(DATA=NS(TASK_KEYS_H5=list(tasks)), MODEL=model, TRAIN=NS(PHASE1_MASK_NULL_LOSS=phase1),
              LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=cls_train, VAL=cls_val)), TASK_SPECIFIC=NS(TRAIN=NS(FUNCS=funcs_train), VAL=NS(FUNCS=funcs_val))))


def test_get_loss_function_name_table_and_class_weight_switch():
    from linnaeus_amd import loss as LS

    cfg = make_config(None, None, smoothing=0.25)
    cwd = {0: 2.0, 3: 0.5, "1": 1.5}
    ce = LS.get_loss_function("CrossEntropyLoss", cfg, cwd, True, "taxa_L10", None, 0)
    assert type(ce) is LS.CrossEntropyLoss and ce.apply_class_weights is True and ce.ignore_index == 0
    assert ce.weight.dtype == torch.float32 and ce.weight.tolist() == [2.0, 1.5, 1.0, 0.5]  # [max index + 1], missing entries 1.0
    val = LS.get_loss_function("CrossEntropyLoss", cfg, cwd, False, "taxa_L10")
    assert val.apply_class_weights is False and val.weight is None and val.ignore_index is None  # CLASS.VAL = False: the dict is not converted
    t = torch.ones(5)
    assert LS.get_loss_function("SoftTargetCrossEntropy", cfg, t, False).weight is t  # a tensor is passed on whatever the switch says
    ls = LS.get_loss_function("LabelSmoothingCrossEntropy", cfg, None, True, ignore_index=0)
    assert type(ls) is LS.LabelSmoothingCrossEntropy and ls.smoothing == 0.25 and ls.weight is None and ls.ignore_index == 0 and ls.config is cfg
    assert LS.get_loss_function("LabelSmoothingCrossEntropy", make_config(None, None), None).smoothing == 0.1
    st = LS.get_loss_function("SoftTargetCrossEntropy", cfg, cwd, True, ignore_index=0)
    assert type(st) is LS.SoftTargetCrossEntropy and st.weight.tolist() == [2.0, 1.5, 1.0, 0.5] and not hasattr(st, "ignore_index")
    tax = LS.get_loss_function("TaxonomyAwareLabelSmoothing", cfg, cwd, True, "taxa_L10", {"taxa_L10": torch.eye(4)}, 0)
    assert type(tax) is LS.TaxonomyAwareLabelSmoothingCE and tax.num_classes == 4 and tax.ignore_index == 0 and tax.weight.tolist() == [2.0, 1.5, 1.0, 0.5]
    with pytest.raises(ValueError, match="task_key"):
        LS.get_loss_function("TaxonomyAwareLabelSmoothing", cfg, None, True, None, {"taxa_L10": torch.eye(4)})
    with pytest.raises(ValueError, match="taxa_L20"):
        LS.get_loss_function("TaxonomyAwareLabelSmoothing", cfg, None, True, "taxa_L20", {"taxa_L10": torch.eye(4)})
    with pytest.raises(ValueError, match="FocalLoss"):
        LS.get_loss_function("FocalLoss", cfg)


def test_prepare_loss_functions():
    from linnaeus_amd import loss as LS

    cfg = make_config(["CrossEntropyLoss", "LabelSmoothingCrossEntropy"], "SoftTargetCrossEntropy", cls_train=True, cls_val=True, phase1=True)
    cw_train = {"taxa_L10": {0: 2.0, 1: 3.0}}
    cw_val = {"taxa_L10": {0: 4.0}, "taxa_L20": {2: 5.0}}
    train, val = LS.prepare_loss_functions(cfg, cw_train, cw_val)
    assert list(train) == list(val) == ["taxa_L10", "taxa_L20"]
    assert type(train["taxa_L10"]) is LS.CrossEntropyLoss and type(train["taxa_L20"]) is LS.LabelSmoothingCrossEntropy
    assert train["taxa_L10"].ignore_index == 0 and train["taxa_L20"].ignore_index == 0  # PHASE1_MASK_NULL_LOSS
    assert train["taxa_L10"].weight.tolist() == [2.0, 3.0] and train["taxa_L20"].weight is None
    assert all(type(v) is LS.SoftTargetCrossEntropy for v in val.values())  # one name for every task
    assert val["taxa_L10"].weight.tolist() == [4.0] and val["taxa_L20"].weight.tolist() == [1.0, 1.0, 5.0]
    train, _ = LS.prepare_loss_functions(make_config("CrossEntropyLoss", "CrossEntropyLoss"), None, None)  # the reference's default configuration
    assert train["taxa_L20"].ignore_index is None and train["taxa_L20"].weight is None
    with pytest.raises(ValueError, match="TRAIN.FUNCS"):
        LS.prepare_loss_functions(make_config(["CrossEntropyLoss"], "CrossEntropyLoss"))


# stand-ins that carry the reference's class names and attributes (loss/basic_loss.py, loss/taxonomy_label_smoothing.py)
def _make(name, attrs):
    obj = type(name, (torch.nn.Module,), {})()
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def test_convert_criteria():
    from linnaeus_amd import loss as LS

    w = torch.tensor([1.0, 2.0, 3.0])
    cfg = object()
    theirs = {
        "taxa_L10": _make("CrossEntropyLoss", dict(weight=w, apply_class_weights=True, ignore_index=0, criterion=None)),
        "taxa_L20": _make("LabelSmoothingCrossEntropy", dict(weight=None, smoothing=0.2, confidence=0.8, apply_class_weights=False, ignore_index=None, config=cfg)),
        "taxa_L30": _make("SoftTargetCrossEntropy", dict(weight=w, apply_class_weights=True)),
        "taxa_L40": _make("TaxonomyAwareLabelSmoothingCE", dict(soft_labels=torch.eye(3), weight=w, apply_class_weights=True, ignore_index=0, config=cfg, num_classes=3)),
    }
    ours = LS.convert_criteria(theirs)
    assert list(ours) == list(theirs)
    a, b, c, d = (ours[t] for t in theirs)
    assert type(a) is LS.CrossEntropyLoss and a.weight is w and a.apply_class_weights is True and a.ignore_index == 0
    assert type(b) is LS.LabelSmoothingCrossEntropy and b.smoothing == 0.2 and b.weight is None and b.apply_class_weights is False and b.ignore_index is None and b.config is cfg
    assert type(c) is LS.SoftTargetCrossEntropy and c.weight is w and c.apply_class_weights is True
    assert type(d) is LS.TaxonomyAwareLabelSmoothingCE and torch.equal(d.soft_labels, torch.eye(3)) and torch.equal(d.weight, w) and d.ignore_index == 0 and d.config is cfg
    # the project's own classes and torch.nn.CrossEntropyLoss come back unchanged
    plain = torch.nn.CrossEntropyLoss(reduction="none")
    again = LS.convert_criteria({**ours, "taxa_L50": plain})
    assert all(again[t] is ours[t] for t in ours) and again["taxa_L50"] is plain
    assert LS.convert_criteria(a) is a
    # anything else is refused by name
    with pytest.raises(L.LnxError, match="MSELoss"):
        LS.convert_criteria({"taxa_L10": torch.nn.MSELoss()})
    with pytest.raises(L.LnxError, match="smoothing"):
        LS.convert_criteria({"taxa_L10": _make("LabelSmoothingCrossEntropy", dict(weight=None, apply_class_weights=False, ignore_index=None))})


def test_fused_loss_accepts_the_classes_and_names_them_when_it_refuses():
    from linnaeus_amd.loss import (CrossEntropyLoss, FusedHierarchicalLoss, GradientWeighting, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy,
                                   TaxonomyAwareLabelSmoothingCE)

    tasks = [f"taxa_L{10 * (i + 1)}" for i in range(8)]
    crit = {t: k for t, k in zip(tasks, [CrossEntropyLoss(), LabelSmoothingCrossEntropy(), SoftTargetCrossEntropy(), TaxonomyAwareLabelSmoothingCE(torch.eye(3)),
                                         torch.nn.CrossEntropyLoss(reduction="none"), SoftTargetCrossEntropy(torch.ones(3), True),
                                         LabelSmoothingCrossEntropy(torch.ones(3), 0.0, True, 0), CrossEntropyLoss(torch.ones(3), True, 0)])}
    FusedHierarchicalLoss(tasks, crit, GradientWeighting(tasks, None, "static"))  # 8 tasks, all five forms
    gw = GradientWeighting(["taxa_L10"], None, "static")
    with pytest.raises(L.LnxError) as e:
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": torch.nn.MSELoss()}, gw)
    for name in ("MSELoss", "TaxonomyAwareLabelSmoothingCE", "CrossEntropyLoss", "LabelSmoothingCrossEntropy", "SoftTargetCrossEntropy", "torch.nn.CrossEntropyLoss"):
        assert name in str(e.value), name
    # torch.nn.CrossEntropyLoss keeps its refusals
    with pytest.raises(L.LnxError, match="class weight"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": torch.nn.CrossEntropyLoss(reduction="none", weight=torch.ones(3))}, gw)
    with pytest.raises(L.LnxError, match="reduction"):
        FusedHierarchicalLoss(["taxa_L10"], {"taxa_L10": torch.nn.CrossEntropyLoss()}, gw)


# ------------------------------------------------------------------------------------------------------------------ host refusals
FAKE = 0x1000  # never dereferenced: every case below is refused on the host


def softce_args(form, C_=5):
    a = L.SoftCEArgs()
    a.B, a.C, a.logits, a.ld, a.target, a.smoothing, a.ignore_index, a.scale = 4, C_, FAKE, 8, FAKE, 0.1, -1, 1.0
    a.loss, a.dlogits, a.ldd, a.form = FAKE, FAKE, 8, form
    if form == L.CE_FORM_SOFT_ROW:
        a.target, a.smoothing, a.soft_target, a.ldt = None, 0.0, FAKE, 8
    return a


SOFTCE_REFUSALS = [
    (L.CE_FORM_OFF_TARGET, dict(C=1, ld=8), b"C >= 2"),
    (L.CE_FORM_OFF_TARGET, dict(soft=FAKE), b"soft matrix"),
    (L.CE_FORM_SOFT_ROW, dict(soft_target=None), b"needs soft_target"),
    (L.CE_FORM_SOFT_ROW, dict(ldt=4), b"ldt=4"),
    (L.CE_FORM_SOFT_ROW, dict(soft=FAKE), b"soft matrix"),
    (L.CE_FORM_SOFT_ROW, dict(ignore_index=0), b"ignore_index"),
    (3, dict(), b"form=3"),
    (-1, dict(), b"form=-1"),
    (L.CE_FORM_DEFAULT, dict(target=None), b"null operand"),  # as before: the class indices are needed unless the rows replace them
    (L.CE_FORM_OFF_TARGET, dict(target=None), b"null operand"),
]


@pytest.mark.parametrize("entry", ["lnx_softce", "lnx_softce_multi"])
def test_softce_refuses_the_new_forms_bad_arguments_before_any_launch(entry):
    lib = L.lib()
    assert lib.lnx_version() >= 110
    for i, (form, spoil, word) in enumerate(SOFTCE_REFUSALS):
        if entry == "lnx_softce":
            a = softce_args(form)
            tgt, ref = a, C.byref(a)
            call = lambda: lib.lnx_softce(ref, None)  # noqa: E731
        else:  # the spoiled set is the second of two
            arr = (L.SoftCEArgs * 2)(softce_args(L.CE_FORM_DEFAULT), softce_args(form))
            tgt = arr[1]
            call = lambda: lib.lnx_softce_multi(arr, 2, None)  # noqa: E731
        for k, v in spoil.items():
            setattr(tgt, k, v)
        assert call() != 0, (i, form, spoil)
        msg = lib.lnx_last_error()
        assert msg.startswith(entry.encode() + b":") and word in msg, (i, msg)


def hier_args(form):
    a = L.HierLossArgs()
    a.dtype, a.B, a.n_tasks, a.prob, a.mask_mul = L.F32, 4, 2, 1.0, 0
    a.draws, a.weights, a.ws, a.out, a.counts = None, FAKE, FAKE, FAKE, FAKE
    for t in range(2):
        k = a.task[t]
        k.logits, k.ld, k.C, k.target, k.soft, k.smoothing, k.ignore_index = FAKE, 8, 5, FAKE, None, 0.0, -1
        k.class_weight, k.n_cw, k.p_cw, k.p_w, k.dlogits, k.ldd = FAKE, 5, 1, 2, FAKE, 8
    k = a.task[1]
    k.form = form
    if form == L.CE_FORM_SOFT_ROW:
        k.target, k.soft_target, k.ldt = None, FAKE, 8
    return a


HIER_REFUSALS = [
    (L.CE_FORM_OFF_TARGET, dict(C=1), b"C >= 2"),
    (L.CE_FORM_OFF_TARGET, dict(soft=FAKE), b"soft matrix"),
    (L.CE_FORM_SOFT_ROW, dict(soft_target=None, target=FAKE), b"needs soft_target"),
    (L.CE_FORM_SOFT_ROW, dict(ldt=4), b"ldt=4"),
    (L.CE_FORM_SOFT_ROW, dict(soft=FAKE), b"soft matrix"),
    (L.CE_FORM_SOFT_ROW, dict(ignore_index=0), b"ignore_index"),
    (3, dict(), b"form=3"),
]


@pytest.mark.parametrize("entry", ["lnx_hier_loss_fwd", "lnx_hier_loss_bwd"])
def test_hier_loss_refuses_the_new_forms_bad_arguments_before_any_launch(entry):
    lib = L.lib()
    call = (lambda a: lib.lnx_hier_loss_fwd(a, None)) if entry == "lnx_hier_loss_fwd" else (lambda a: lib.lnx_hier_loss_bwd(a, C.c_void_p(FAKE), None))
    for i, (form, spoil, word) in enumerate(HIER_REFUSALS):
        a = hier_args(form)
        for k, v in spoil.items():
            setattr(a.task[1], k, v)
        assert call(C.byref(a)) != 0, (i, form, spoil)
        msg = lib.lnx_last_error()
        assert msg.startswith(entry.encode() + b":") and word in msg and b"task 1" in msg, (i, msg)


# ------------------------------------------------------------------------------------------------------------------ the struct mirrors
def test_grown_structs_match_the_c_compiler(tmp_path):
    """sizeof and the offset of every appended field of the two structs that grew, from a gcc-compiled probe of include/lnx.h"""
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    probes = [("lnx_softce_args", L.SoftCEArgs, ("ldd", "form", "soft_target", "ldt")), ("lnx_hier_loss_task", L.HierLossTask, ("ldd", "form")),
              ("lnx_hier_loss_args", L.HierLossArgs, ("task",))]
    lines = []
    for name, _, fields in probes:
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));\n')
        lines += [f'    printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n' for f in fields]
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "lnx.h"\nint main(void) {\n' + "".join(lines) +
                   '    printf("forms %d %d %d\\n", LNX_CE_FORM_DEFAULT, LNX_CE_FORM_OFF_TARGET, LNX_CE_FORM_SOFT_ROW);\n    return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
               if not line.startswith("forms"))
    for name, cls, fields in probes:
        assert int(got[name]) == C.sizeof(cls), (name, got[name], C.sizeof(cls))
        for f in fields:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert f"forms {L.CE_FORM_DEFAULT} {L.CE_FORM_OFF_TARGET} {L.CE_FORM_SOFT_ROW}" in out
    # a zero-filled struct selects today's forms
    assert L.SoftCEArgs().form == L.CE_FORM_DEFAULT == 0 and L.HierLossTask().form == 0 and not L.SoftCEArgs().soft_target
