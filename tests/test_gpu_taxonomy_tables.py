"""The taxonomy smoothing tables on the GPU: lnx_taxonomy_rows against the numpy restatement (tests/taxonomy_ref.py), the table form
LNX_CE_FORM_TAXONOMY of lnx_softce / lnx_softce_multi / lnx_hier_loss_fwd / lnx_hier_loss_bwd bit for bit against the matrix form on
the matrix `tables.dense()` gives, TaxonomyAwareLabelSmoothingCE.from_tables against the reference criterion's recorded values
(tests/golden/taxonomy_tables.npz) and, at 50 000 classes, against an fp64 evaluation, the wiring, and the argument checks."""
import ctypes as C
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import linnaeus_amd
from linnaeus_amd import _lib as L
from linnaeus_amd import loss as LS
from tests import taxonomy_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = (2, 255, 256, 257, 1000)  # one class pair; one short of, exactly, one past the 256 columns of a pass; several passes
B = 5
NAN = float("nan")


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    linnaeus_amd.set_deterministic(False)


_TABLES = {}


def tables_for(Cn, D, setting=(0.1, 1.0, False)):
    """seeded forest with Cn finest classes under D further levels (each a quarter of the one below, at least 2 classes).  Without
    uniform_roots the parentless class 1 is a uniform-FALLBACK row (its weight sum is 0), as is the only child 3 of a parentless parent"""
    key = (Cn, D, setting)
    if key not in _TABLES:
        ncls = [Cn] + [max(2, -(-Cn // 4 ** k)) for k in range(1, D + 1)]
        parents = R.random_forest(np.random.default_rng(1000 * D + Cn), ncls)
        _TABLES[key] = LS.build_taxonomy_smoothing_tables(parents, ncls, 0, *setting)
    return _TABLES[key]


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------------ lnx_taxonomy_rows
@pytest.mark.parametrize("D", [0, 1, 3, 8])
@pytest.mark.parametrize("Cn", SIZES)
def test_taxonomy_rows_equal_the_restatement(Cn, D):
    t = tables_for(Cn, D)
    anc, val = t.to("cuda")
    g = torch.Generator().manual_seed(Cn + D)
    picked = torch.cat([torch.tensor([Cn - 1, 0, 1 % Cn]), torch.randint(0, Cn, (4,), generator=g)])
    for what, ref in ((0, R.dense(t.anc.numpy(), t.val.numpy())), (1, R.distances(t.anc.numpy()))):
        ref = torch.from_numpy(ref)
        for rows in (None, picked):
            n = Cn if rows is None else len(rows)
            out = torch.full((n, Cn + 3), NAN, device="cuda")  # ldo > C: the sentinels past C must survive
            a = L.TaxonomyRowsArgs()
            a.C, a.depth, a.anc, a.val = Cn, D, anc.data_ptr() or None, val.data_ptr()
            dev_rows = rows.cuda() if rows is not None else None
            a.rows, a.n, a.out, a.ldo, a.what = (dev_rows.data_ptr() if rows is not None else None), n, out.data_ptr(), out.stride(0), what
            L.check(L.lib().lnx_taxonomy_rows(C.byref(a), stream()), "lnx_taxonomy_rows")
            want = ref if rows is None else ref[rows]
            assert torch.equal(out[:, :Cn].cpu(), want), (what, rows is None)
            assert bool(torch.isnan(out[:, Cn:]).all())
            got = (t.dense if what == 0 else t.distances)(rows)  # the public surface: contiguous [n, C]
            assert got.is_cuda and torch.equal(got.cpu(), want)
    if D:
        assert bool(torch.isinf(torch.from_numpy(R.distances(t.anc.numpy()))).any())  # disconnected pairs exist


def test_taxonomy_rows_out_of_range_row_is_nan():
    t = tables_for(257, 3)
    got = t.dense(torch.tensor([5, 257, -1]))
    assert bool(torch.isnan(got[1:]).all()) and torch.equal(got[0].cpu(), torch.from_numpy(R.dense(t.anc.numpy(), t.val.numpy(), [5]))[0])


# ------------------------------------------------------------------------------------------------------------------ bit for bit: lnx_softce
def ce_case(Cn, D):
    t = tables_for(Cn, D)
    g = torch.Generator().manual_seed(77 * Cn + D)
    # the ignored class, an out-of-range class, a parentless class (a uniform-fallback row), the only child of its parent, any class
    target = torch.tensor([0, Cn + 3, 1 % Cn, 3 % Cn if Cn > 3 else 1, int(torch.randint(1, Cn, (1,), generator=g))])
    return NS(t=t, C=Cn, x=(torch.randn(B, Cn, generator=g) * 3).cuda(), target=target.cuda(), cw=(torch.rand(Cn, generator=g) + 0.5).cuda(),
              rs=(torch.rand(B, generator=g) + 0.5).cuda(), soft=t.dense())


def softce_outputs(case, table_form, det):
    """(loss, loss_sum, dlogits) of one launch; dlogits has a NaN sentinel column past C"""
    loss = torch.full((B,), NAN, device="cuda")
    total = torch.zeros((), device="cuda")
    d = torch.full((B, case.C + 1), NAN, device="cuda")
    sum_ws = torch.empty(B, device="cuda") if det else None
    tax = case.t.to("cuda") + (case.t.depth,) if table_form else None
    args = (case.x, case.target, None if table_form else case.soft, 0.0, case.cw, 0, case.rs, 0.37, loss, total, d[:, :case.C],
            L.CE_FORM_TAXONOMY if table_form else L.CE_FORM_DEFAULT, None, sum_ws, tax)
    return args, (loss, total, d)


def check_softce_row_properties(case, loss, d):
    assert float(loss[0]) == 0.0 and bool((d[0, :case.C] == 0).all())              # the ignored class
    assert bool(torch.isnan(loss[1])) and bool((d[1, :case.C] == 0).all())         # out of range: NaN loss, zero gradient row
    assert bool(torch.isfinite(loss[2:]).all()) and bool((d[2:, :case.C].abs().sum(1) > 0).all())
    assert bool(torch.isnan(d[:, case.C]).all())


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("Cn,D", [(c, 3) for c in SIZES] + [(257, 0), (257, 8), (1000, 1)])
def test_softce_table_form_equals_matrix_form_bit_for_bit(Cn, D, det):
    case = ce_case(Cn, D)
    linnaeus_amd.set_deterministic(det)
    res = []
    for table_form in (False, True, True):
        args, outs = softce_outputs(case, table_form, det)
        LS._launch(*args)
        res.append(outs)
    for k, name in enumerate(("loss", "loss_sum", "dlogits")):
        assert same_bits(res[0][k], res[1][k]), name
        assert same_bits(res[1][k], res[2][k]), f"{name}: the table form differs run to run"
    check_softce_row_properties(case, res[1][0], res[1][2])
    # the uniform-fallback row really is one: every off-diagonal entry of row 1 is alpha / (C - 1)
    if Cn > 2:
        row = case.soft[1].cpu()
        assert bool((row[torch.arange(Cn) != 1] == np.float32(0.1 / (Cn - 1))).all())


@pytest.mark.parametrize("det", [False, True])
def test_softce_multi_table_form_equals_matrix_form_bit_for_bit(det):
    cases = [ce_case(c, 3) for c in SIZES]
    linnaeus_amd.set_deterministic(det)
    res = []
    for table_form in (False, True, True):
        sets, outs = zip(*[softce_outputs(c, table_form, det) for c in cases])
        LS._launch_multi(list(sets))
        res.append(outs)
    for i, c in enumerate(cases):
        for k, name in enumerate(("loss", "loss_sum", "dlogits")):
            assert same_bits(res[0][i][k], res[1][i][k]), (c.C, name)
            assert same_bits(res[1][i][k], res[2][i][k]), (c.C, name)
        check_softce_row_properties(c, res[1][i][0], res[1][i][2])


# ------------------------------------------------------------------------------------------------------------------ bit for bit: lnx_hier_loss
def hier_outputs(cases, table_form, dtype, soft_target, det):
    """one lnx_hier_loss_fwd + lnx_hier_loss_bwd over the five sizes as five tasks: (ws, out, counts, [dlogits])"""
    T = len(cases)
    g = torch.Generator().manual_seed(31)
    ws = torch.full((T, L.HL_WS_ROWS, B), NAN, device="cuda")
    out = torch.zeros(L.HL_OUT_FLOATS, device="cuda")
    counts = torch.zeros(L.HL_COUNTS, dtype=torch.int64, device="cuda")
    draws = torch.rand(T, B, generator=g)
    draws[:, 0] = torch.tensor([0.1, 0.9] * T)[:T]  # row 0 is null (class 0) in every task: kept in some, masked in others
    draws = draws.cuda()
    weights = (torch.rand(T, generator=g) + 0.5).cuda()
    a = L.HierLossArgs()
    a.dtype, a.B, a.n_tasks, a.prob, a.mask_mul = (L.BF16 if dtype == torch.bfloat16 else L.F32), B, T, 0.5, 0
    a.draws, a.weights, a.ws, a.out, a.counts = draws.data_ptr(), weights.data_ptr(), ws.data_ptr(), out.data_ptr(), counts.data_ptr()
    keep, dls = [], []
    for i, c in enumerate(cases):
        k = a.task[i]
        x = c.x.to(dtype)
        k.logits, k.ld, k.C = x.data_ptr(), x.stride(0), c.C
        if soft_target:  # 0.7 of the class, 0.3 of its neighbour: the first maximum is the class (an out-of-range class cannot be written)
            cls = c.target.clamp(0, c.C - 1)
            y = 0.7 * torch.nn.functional.one_hot(cls, c.C).float() + 0.3 * torch.nn.functional.one_hot((cls + 1) % c.C, c.C).float()
            k.soft_target, k.ldt = y.data_ptr(), y.stride(0)
            keep.append(y)
        else:
            k.target = c.target.data_ptr()
        if table_form:
            anc, val = c.t.to("cuda")
            k.form, k.tax_anc, k.tax_val, k.tax_depth = L.CE_FORM_TAXONOMY, anc.data_ptr() or None, val.data_ptr(), c.t.depth
        else:
            k.soft = c.soft.data_ptr()
        k.crit_weight, k.ignore_index = c.cw.data_ptr(), (0 if i % 2 == 0 else -1)
        k.class_weight, k.n_cw, k.p_cw, k.p_w = c.cw.data_ptr(), c.C, 1, 2
        d = torch.full((B, c.C + 1), NAN, device="cuda")
        k.dlogits, k.ldd = d.data_ptr(), d.stride(0)
        keep.append(x)
        dls.append(d)
    go = torch.tensor([1.7], device="cuda")
    linnaeus_amd.set_deterministic(det)
    L.check(L.lib().lnx_hier_loss_fwd(C.byref(a), stream()), "lnx_hier_loss_fwd")
    L.check(L.lib().lnx_hier_loss_bwd(C.byref(a), C.c_void_p(go.data_ptr()), stream()), "lnx_hier_loss_bwd")
    torch.cuda.synchronize()
    return ws, out, counts, dls


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("soft_target", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hier_loss_table_form_equals_matrix_form_bit_for_bit(dtype, soft_target, det):
    cases = [ce_case(c, 3) for c in SIZES]
    m = hier_outputs(cases, False, dtype, soft_target, det)
    t1 = hier_outputs(cases, True, dtype, soft_target, det)
    t2 = hier_outputs(cases, True, dtype, soft_target, det)
    for k, name in enumerate(("ws", "out", "counts")):
        assert same_bits(m[k], t1[k]), name
        assert same_bits(t1[k], t2[k]), f"{name}: the table form differs run to run"
    for i, c in enumerate(cases):
        assert same_bits(m[3][i], t1[3][i]) and same_bits(t1[3][i], t2[3][i]), c.C
        assert bool(torch.isnan(t1[3][i][:, c.C]).all()) and not bool(torch.isnan(t1[3][i][:, :c.C]).any())
    ws, out, counts, dls = t1
    flags = ws[:, L.HL_WS_FLAGS].contiguous().view(torch.int32)
    assert bool((flags[:, 0] & 1).all())                                   # row 0 is null everywhere
    kept0 = (flags[:, 0] & 2) != 0
    assert bool(kept0.any()) and not bool(kept0.all())                     # the draws keep it in some tasks and mask it in others
    if not soft_target:
        assert bool(torch.isnan(ws[:, L.HL_WS_RAW, 1]).all())              # the out-of-range class: NaN loss ...
        assert all(bool((d[1, :-1] == 0).all()) for d in dls)              # ... zero gradient row
    assert bool((ws[0::2, L.HL_WS_RAW, 0] == 0).all())                     # tasks with ignore_index = 0
    assert bool((ws[1::2, L.HL_WS_RAW, 0] > 0).all())
    assert bool(torch.isfinite(ws[:, L.HL_WS_RAW, 2:]).all()) and all(bool((d[2:, :-1].abs().sum(1) > 0).all()) for d in dls)


# ------------------------------------------------------------------------------------------------------------------ the reference's numbers
def test_from_tables_matches_the_reference_criterion():
    z = np.load(os.path.join(GOLDEN, "taxonomy_tables.npz"))
    worst_l = worst_g = 0.0
    for f, ncls in enumerate(z["forests"]):
        ncls = [int(c) for c in ncls]
        parents = [z[f"f{f}_parents_{lv}"] for lv in range(len(ncls))]
        for lv in range(len(ncls)):
            x0 = torch.from_numpy(z[f"f{f}_l{lv}_logits"]).cuda()
            target = torch.from_numpy(z[f"f{f}_l{lv}_target"]).cuda()
            cw = torch.from_numpy(z[f"f{f}_l{lv}_cw"])
            for s, (alpha, beta, ur) in enumerate(R.SETTINGS):
                t = LS.build_taxonomy_smoothing_tables(parents, ncls, lv, alpha, beta, ur)
                crit = LS.TaxonomyAwareLabelSmoothingCE.from_tables(t, weight=cw, apply_class_weights=True, ignore_index=0).cuda()
                assert crit.tax_val.is_cuda and crit.tax_anc.is_cuda and crit.class_weight.is_cuda  # .cuda() moved the buffers
                x = x0.clone().requires_grad_(True)
                loss = crit(x, target)
                loss.sum().backward()
                want_l, want_g = z[f"f{f}_l{lv}_s{s}_loss"], z[f"f{f}_l{lv}_s{s}_grad"]
                worst_l = max(worst_l, float(np.abs(loss.detach().cpu().numpy() - want_l).max()))
                worst_g = max(worst_g, float(np.abs(x.grad.cpu().numpy() - want_g).max()))
                np.testing.assert_allclose(loss.detach().cpu().numpy(), want_l, rtol=2e-5, atol=2e-6, err_msg=str((f, lv, s)))
                np.testing.assert_allclose(x.grad.cpu().numpy(), want_g, rtol=2e-4, atol=2e-6, err_msg=str((f, lv, s)))
                assert float(loss.detach()[0]) == 0.0  # class 0 under ignore_index = 0
    print(f"from_tables vs the reference criterion: max abs difference loss {worst_l:.3e}, gradient {worst_g:.3e}")


def test_criterion_at_50000_classes_against_fp64():
    """the matrix would be 10 GB; the criterion holds 2 MB"""
    rng = np.random.default_rng(5)
    ncls = [50_000, 6_000, 700, 80, 9]
    parents = [rng.integers(0, ncls[lv + 1], ncls[lv]) for lv in range(4)]
    for p in parents:
        p[7] = -1  # a parentless class per level
    t = LS.build_taxonomy_smoothing_tables(parents, ncls, 0, 0.1, 1.0, True, keep_fp64=True)
    cw = torch.from_numpy(rng.random(ncls[0]).astype(np.float32) + 0.5)
    crit = LS.TaxonomyAwareLabelSmoothingCE.from_tables(t, weight=cw, apply_class_weights=True, ignore_index=0).cuda()
    assert crit.soft_labels is None and sum(b.numel() * b.element_size() for b in (crit.tax_anc, crit.tax_val)) == 2_000_000
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(4, ncls[0], generator=g) * 2).cuda().requires_grad_(True)
    target = torch.tensor([0, 7, 49_999, 12_345]).cuda()
    loss = crit(x, target)
    loss.sum().backward()
    S = R.dense(t.anc.numpy(), t.val.numpy().astype(np.float64), target.cpu().numpy())
    want_l, want_g = R.soft_ce(x.detach().cpu().numpy(), S, target.cpu().numpy(), cw.numpy(), 0)
    np.testing.assert_allclose(loss.detach().cpu().numpy(), want_l, rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), want_g, rtol=2e-4, atol=2e-6)
    assert float(loss.detach()[0]) == 0.0 and bool((loss[1:] > 0).all())
    with pytest.raises(IndexError, match="1 target indices out of bounds"):  # validate_targets behaves as in the matrix form
        crit(x.detach(), torch.tensor([0, 50_000, 1, 2]).cuda())


# ------------------------------------------------------------------------------------------------------------------ wiring
def wiring_case(table_form):
    from tests.test_gpu_hier_loss import CFG

    heads = (("taxa_L10", 257), ("taxa_L20", 65), ("taxa_L30", 17), ("taxa_L40", 5))
    ncls = [c for _, c in heads]
    parents = R.random_forest(np.random.default_rng(3), ncls)
    g = torch.Generator().manual_seed(4)
    tasks = [t for t, _ in heads]
    base, tg, crit, cw = {}, {}, {}, {}
    for lv, (t, c) in enumerate(heads):
        base[t] = (torch.randn(33, c, generator=g) * 2).cuda()
        y = torch.randint(0, c, (33,), generator=g)
        y[:9] = 0
        tg[t] = y.cuda()
        if lv in (0, 2):  # two tasks with taxonomy smoothing, two with plain cross entropy
            tab = LS.build_taxonomy_smoothing_tables(parents, ncls, lv, 0.2, 0.5, True)
            crit[t] = (LS.TaxonomyAwareLabelSmoothingCE.from_tables(tab) if table_form else LS.TaxonomyAwareLabelSmoothingCE(tab.dense())).cuda()
            crit[t].validate_targets = False
        else:
            crit[t] = LS.CrossEntropyLoss()
        cw[t] = {i: float(0.5 + torch.rand(1, generator=g).item()) for i in range(0, c, 2)}
    tw = {t: float(0.3 + torch.rand(1, generator=g).item()) for t in tasks}
    gw = LS.GradientWeighting(tasks, CFG, "static", init_weights=tw, class_weights=cw).cuda()
    coin = {t: torch.rand(33, generator=g).cuda() for t in tasks}
    return NS(tasks=tasks, base=base, tg=tg, crit=crit, gw=gw, cfg=CFG, B=33), coin


def test_weighted_hierarchical_loss_takes_table_form_criteria():
    from tests.test_gpu_hier_loss import assert_same_as_composed, run_path

    case, coin = wiring_case(True)
    f = run_path(case, True, 0.5, coin=coin)
    c = run_path(case, False, 0.5, coin=coin)
    assert_same_as_composed(f, c, case.tasks, 33)
    mcase, _ = wiring_case(False)  # the same criteria over the dense matrices: the same bits on both paths
    for fused, tab in ((True, f), (False, c)):
        mat = run_path(mcase, fused, 0.5, coin=coin)
        assert same_bits(mat.total, tab.total), fused
        assert all(same_bits(mat.grads[t], tab.grads[t]) for t in case.tasks), fused
    lg = {t: {"logits": case.base[t]} for t in case.tasks}  # dict-valued head outputs stay refused by the fused path
    with pytest.raises(L.LnxError, match="dict-valued head outputs"):
        LS.weighted_hierarchical_loss(lg, case.tg, case.crit, case.gw, NS(get_null_mask_prob=lambda s: 0.5), 0, config=case.cfg, fused=True)


def test_prepare_loss_functions_builds_table_form_criteria():
    keys = ["taxa_L10", "taxa_L20"]
    ncls = [40, 9]
    parents = R.random_forest(np.random.default_rng(8), ncls)
    tab = {"taxa_L10": LS.build_taxonomy_smoothing_tables(parents, ncls, 0)}
    funcs = ["TaxonomyAwareLabelSmoothing", "CrossEntropyLoss"]
    cfg = NS(DATA=NS(TASK_KEYS_H5=keys), TRAIN=NS(PHASE1_MASK_NULL_LOSS=True),
             LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=False, VAL=False)), TASK_SPECIFIC=NS(TRAIN=NS(FUNCS=funcs), VAL=NS(FUNCS=funcs))))
    train, val = LS.prepare_loss_functions(cfg, taxonomy_matrices=tab)
    crit = train["taxa_L10"]
    assert crit.soft_labels is None and crit.ignore_index == 0 and val["taxa_L10"].soft_labels is None
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(6, 40, generator=g).cuda(), torch.randint(0, 40, (6,), generator=g).cuda()
    want = LS.TaxonomyAwareLabelSmoothingCE(tab["taxa_L10"].dense(), ignore_index=0)(x, y)
    assert same_bits(crit(x, y), want)
    assert same_bits(crit(x, torch.nn.functional.one_hot(y, 40).float()), want)  # [B, C] targets are arg-maxed, as in the matrix form


def test_gradnorm_per_task_path_accepts_table_form():
    from linnaeus_amd import build_model
    from oracle import mformer_oracle as O
    from tests.cases import CASES, SEED, model_state_dict_from_oracle
    from tests.test_gradnorm import gradnorm_cfg

    spec = CASES["tiny_a"]
    tasks, ncls = [t for t, _ in spec.heads], [c for _, c in spec.heads]
    parents = R.random_forest(np.random.default_rng(12), ncls)
    tabs = {t: LS.build_taxonomy_smoothing_tables(parents, ncls, lv, 0.2, 0.5, True) for lv, t in enumerate(tasks)}
    cfg = gradnorm_cfg(spec)
    model = build_model(cfg, num_classes=dict(spec.heads))
    model.load_state_dict(model_state_dict_from_oracle(model, O.seeded_state_dict(O.param_shapes(spec), SEED)), strict=True)
    model = model.cuda().train()
    model.set_compute_dtype("fp32")
    x, meta = O.seeded_inputs(spec, 4, 64, SEED + 100)
    g = torch.Generator().manual_seed(1)
    targets = {t: torch.randint(0, c, (4,), generator=g).cuda() for t, c in spec.heads}
    res = []
    for table_form in (False, True):
        crit = {t: (LS.TaxonomyAwareLabelSmoothingCE.from_tables(tabs[t]) if table_form else LS.TaxonomyAwareLabelSmoothingCE(tabs[t].dense())).cuda()
                for t in tasks}
        gw = LS.GradientWeighting(tasks, cfg, "gradnorm", alpha=1.5)
        gw.set_model(model)
        res.append(gw.update_gradnorm_weights_reforward((x.cuda(), targets, meta.cuda()), crit, amp_enabled=False, current_step=0))
    assert set(res[0]) == set(res[1]) and any("/norm/" in k for k in res[1])
    for k, v in res[0].items():  # the seeds have the same bits; the backbone norms behind them are summed by float atomics
        assert res[1][k] == pytest.approx(v, rel=2e-4, abs=1e-6), k


# ------------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_refuse_and_launch_nothing():
    case = ce_case(257, 3)
    anc, val = case.t.to("cuda")
    lib = L.lib()

    def softce_args(**kw):
        a = L.SoftCEArgs()
        args, outs = softce_outputs(case, True, False)
        LS._fill(a, *args)
        for k, v in kw.items():
            setattr(a, k, v)
        return a, outs

    def hier_args(**kw):
        a = L.HierLossArgs()
        ws, out = torch.full((L.HL_WS_ROWS, B), NAN, device="cuda"), torch.full((L.HL_OUT_FLOATS,), NAN, device="cuda")
        counts, w = torch.full((L.HL_COUNTS,), -7, dtype=torch.int64, device="cuda"), torch.ones(1, device="cuda")
        d = torch.full((B, 257), NAN, device="cuda")
        a.B, a.n_tasks, a.prob, a.weights, a.ws, a.out, a.counts = B, 1, 1.0, w.data_ptr(), ws.data_ptr(), out.data_ptr(), counts.data_ptr()
        k = a.task[0]
        k.logits, k.ld, k.C, k.target, k.ignore_index = case.x.data_ptr(), 257, 257, case.target.data_ptr(), -1
        k.form, k.tax_anc, k.tax_val, k.tax_depth, k.dlogits, k.ldd = L.CE_FORM_TAXONOMY, anc.data_ptr(), val.data_ptr(), 3, d.data_ptr(), 257
        for key, v in kw.items():
            setattr(k, key, v)
        return a, (ws, out, d, w)

    go = torch.ones(1, device="cuda")
    for kw, words in (({"soft": case.soft.data_ptr()}, b"excludes a [C, C] soft matrix"), ({"tax_depth": 9}, b"tax_depth=9"), ({"tax_val": None}, b"needs tax_val")):
        for who, call in (("lnx_softce", lambda a: lib.lnx_softce(C.byref(a), stream())), ("lnx_softce_multi", lambda a: lib.lnx_softce_multi(C.byref(a), 1, stream()))):
            a, (loss, total, d) = softce_args(**kw)
            assert call(a) != 0, (who, kw)
            msg = lib.lnx_last_error()
            assert who.encode() in msg and words in msg, msg
            torch.cuda.synchronize()
            assert bool(torch.isnan(loss).all()) and float(total) == 0.0 and bool(torch.isnan(d).all())  # nothing was launched
        for who, call in (("lnx_hier_loss_fwd", lambda a: lib.lnx_hier_loss_fwd(C.byref(a), stream())),
                          ("lnx_hier_loss_bwd", lambda a: lib.lnx_hier_loss_bwd(C.byref(a), C.c_void_p(go.data_ptr()), stream()))):
            a, (ws, out, d, w) = hier_args(**kw)
            assert call(a) != 0, (who, kw)
            msg = lib.lnx_last_error()
            assert who.encode() in msg and words in msg, msg
            torch.cuda.synchronize()
            assert bool(torch.isnan(ws).all()) and bool(torch.isnan(out).all()) and bool(torch.isnan(d).all())
    out = torch.full((3, 257), NAN, device="cuda")
    a = L.TaxonomyRowsArgs()
    a.C, a.depth, a.anc, a.val, a.n, a.out, a.ldo, a.what = 257, 9, anc.data_ptr(), val.data_ptr(), 3, out.data_ptr(), 257, 0
    assert lib.lnx_taxonomy_rows(C.byref(a), stream()) != 0 and b"depth=9" in lib.lnx_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
