"""GradNorm on the MI355X: repeated lnx_plan_backward_into after one forward, the lnx_gradnorm_update / lnx_gradnorm_sumsq kernels
against the reference's known answers, and whole updates against tests/golden/gradnorm.npz (the reference's
update_gradnorm_weights_reforward on the same tiny model, fp32 on CPU).

Tolerances.  fp32 plans match the reference's logits to rtol 1e-4 (test_gpu_model); a backbone gradient norm is a root of a sum of
squares of ~4e5 fp32 terms, so its relative error is about the gradients' own (~1e-5..1e-4): norms and losses rtol 2e-4.  A weight
is norm / target, renormalised, with target ~ g_avg r^alpha: its relative error is at most (2 + alpha) times the norms' -- rtol 1e-3.
The update kernel alone, fed the reference's inputs, differs from torch only in the rounding of single fp32 operations: rtol 2e-6."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from linnaeus_amd.loss import GradientWeighting, TaxonomyAwareLabelSmoothingCE, gradnorm_desc_table, weighted_hierarchical_loss
from oracle import mformer_oracle as O
from tests.cases import CASES, SEED, make_config, model_state_dict_from_oracle
from tests.test_gradnorm import gradnorm_cfg

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPEC = CASES["tiny_a"]
TASKS = [t for t, _ in SPEC.heads]


def tiny(dtype="fp32", cfg=None, grad_mode="autograd"):
    sd = O.seeded_state_dict(O.param_shapes(SPEC), SEED)
    model = build_model(cfg or gradnorm_cfg(SPEC), num_classes={t: c for t, c in SPEC.heads})
    model.grad_mode = grad_mode
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype(dtype)
    return model


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("recompute", [False, True])
def test_backward_into_repeats_after_one_forward(recompute):
    """k = 3 lnx_plan_backward_into after ONE forward each equal a fresh forward + backward (up to the float atomics of the
    LayerNorm column sums), and leave the bound arena and every .grad bit for bit as they were."""
    model = tiny()
    model.train()
    x, meta = O.seeded_inputs(SPEC, 4, 64, SEED + 1)
    x, meta = x.cuda(), meta.cuda()
    O.probe_loss(model(x, meta, force_checkpointing=recompute)).backward()  # the step's own gradients
    torch.cuda.synchronize()
    arena0 = model._grad_arena.clone()
    grads0 = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    st = model._get_plan(4, 64, 64, True, recompute)
    model._active = st
    _, logits = model._plan_forward(x, meta, None)
    dl = torch.zeros_like(logits)
    ramps = []
    for i, v in enumerate(model._task_views(st, dl, 4)):
        r = torch.sin(torch.arange(v.numel(), device="cuda", dtype=torch.float32).reshape(v.shape) * 0.37 + i)
        v.copy_(r)
        ramps.append(r)
    rows = torch.zeros(3, model._grad_arena.numel(), device="cuda")
    base = model._grad_arena.data_ptr()
    offs = [v.data_ptr() - base for v in model._grad_views]
    for k in range(3):
        ptrs = (C.c_void_p * st["n"])(*[rows[k].data_ptr() + o for o in offs])
        L.check(L.lib().lnx_plan_backward_into(st["handle"], C.c_void_p(dl.data_ptr()), None, ptrs, stream()), "lnx_plan_backward_into")
    torch.cuda.synchronize()
    assert torch.equal(model._grad_arena, arena0)
    for n, p in model.named_parameters():
        if n in grads0:
            assert torch.equal(p.grad, grads0[n]), n
    # fresh forward + backward of the same seed through autograd
    out = model(x, meta, force_checkpointing=recompute)
    loss = sum((out[t] * r).sum() for t, r in zip(st["tasks"], ramps))
    ref = torch.autograd.grad(loss, st["params"])
    for k in range(3):
        for i, (g, p) in enumerate(zip(ref, st["params"])):
            got = rows[k][offs[i] // 4: offs[i] // 4 + p.numel()].view(p.shape)
            scale = float(g.abs().max()) + 1e-30
            torch.testing.assert_close(got, g, rtol=1e-4, atol=2e-5 * scale, msg=lambda m: f"call {k} {st['names'][i]}: {m}")


def _update(T, alpha, norm, loss, weights, initial, initted, init_loss=None):
    dev = "cuda"
    nrm = torch.tensor(norm, device=dev, dtype=torch.float32)
    ls = torch.tensor(loss, device=dev, dtype=torch.float32)
    cnt = torch.ones(T, device=dev)
    metrics = torch.empty(1 + 5 * T, device=dev)
    a = L.GradNormArgs()
    a.T, a.alpha = T, alpha
    a.norm, a.loss_sum, a.count, a.init_loss = nrm.data_ptr(), ls.data_ptr(), cnt.data_ptr(), None
    a.weights, a.initial_losses, a.initted, a.metrics = weights.data_ptr(), initial.data_ptr(), initted.data_ptr(), metrics.data_ptr()
    L.check(L.lib().lnx_gradnorm_update(C.byref(a), stream()), "lnx_gradnorm_update")
    return metrics.cpu()


@pytest.mark.parametrize("case", ["k0", "k1", "k2"])
def test_update_kernel_reproduces_measure_and_update(case):
    z = np.load(os.path.join(GOLDEN, "gradnorm.npz"), allow_pickle=False)
    keys = [str(k) for k in z[f"{case}_keys"]]
    order = sorted(range(len(keys)), key=lambda i: keys[i])
    srt = [keys[i] for i in order]
    T, alpha = len(keys), float(z[f"{case}_alpha"])
    # measure_and_update indexes task_weights by sorted key: the buffer holds INIT_WEIGHTS in that order (the quirk)
    weights = torch.tensor(z[f"{case}_init"], device="cuda")
    initial = torch.zeros(T, device="cuda")
    initted = torch.zeros(1, device="cuda", dtype=torch.int32)
    for call in range(2):
        m = _update(T, alpha, z[f"{case}_{call}_norm"][order].tolist(), z[f"{case}_{call}_loss"][order].tolist(), weights, initial, initted)
        np.testing.assert_allclose(weights.cpu().numpy(), z[f"{case}_{call}_weights"], rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(initial.cpu().numpy(), z[f"{case}_{call}_initial_losses"], rtol=2e-6)
        got = {"gradnorm/avg_norm": float(m[0])}
        kinds = ("loss", "norm", "target", "weight") + (("ratio",) if alpha > 0 else ())
        for j, kind in enumerate(kinds):
            for i, k in enumerate(srt):
                got[f"gradnorm/{kind}/{k}"] = float(m[1 + j * T + i])
        want = dict(zip([str(k) for k in z[f"{case}_{call}_metric_keys"]], z[f"{case}_{call}_metrics"]))
        assert set(got) == set(want)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=2e-6, abs=1e-6), (call, k)
    assert int(initted.item()) == (1 if alpha > 0 else 0)


def test_sumsq_kernel_matches_grad_sumsq_bitwise_and_float64():
    g = torch.Generator(device="cuda").manual_seed(5)
    T, total = 3, 50_003 * 4
    arenas = torch.randn(T, total, device="cuda", generator=g)
    slices = [(0, 4099), (4100, 1), (4104, 70_001), (80_000, 120_000)]
    arr, blk = gradnorm_desc_table(slices, arenas.data_ptr())
    table = torch.frombuffer(bytearray(arr), dtype=torch.uint8).cuda()
    ws = torch.empty(T * blk, device="cuda")
    sumsq, norm = torch.empty(T, device="cuda"), torch.empty(T, device="cuda")
    L.check(L.lib().lnx_gradnorm_sumsq(C.c_void_p(table.data_ptr()), len(slices), blk, T, arenas.stride(0), C.c_void_p(sumsq.data_ptr()),
                                       C.c_void_p(norm.data_ptr()), C.c_void_p(ws.data_ptr()), stream()), "lnx_gradnorm_sumsq")
    for t in range(T):
        arr_t, _ = gradnorm_desc_table(slices, arenas[t].data_ptr())
        tab_t = torch.frombuffer(bytearray(arr_t), dtype=torch.uint8).cuda()
        one, ws1 = torch.empty(1, device="cuda"), torch.empty(blk, device="cuda")
        L.check(L.lib().lnx_grad_sumsq(C.c_void_p(tab_t.data_ptr()), len(slices), blk, C.c_void_p(one.data_ptr()), C.c_void_p(ws1.data_ptr()), stream()),
                "lnx_grad_sumsq")
        assert float(one) == float(sumsq[t])  # same fold: the same bits as the clip's norm
        want = sum(float((arenas[t, o:o + n].double() ** 2).sum()) for o, n in slices)
        assert float(sumsq[t]) == pytest.approx(want, rel=1e-5)
        assert float(norm[t]) == pytest.approx(want ** 0.5, rel=1e-5)


def soft_criteria(z):
    return {t: TaxonomyAwareLabelSmoothingCE(torch.from_numpy(z[f"soft_{t}"])).cuda() for t in TASKS}


CASE_CFG = {"c0": dict(ALPHA=1.5, ZERO_AUX_INFO=True, GRADNORM_ACCUM_STEPS=1, ckpt=True),
            "c1": dict(ALPHA=0.0, ZERO_AUX_INFO=False, GRADNORM_ACCUM_STEPS=2, ckpt=False),
            "c2": dict(ALPHA=1.5, ZERO_AUX_INFO=False, GRADNORM_ACCUM_STEPS=2, ckpt=True)}


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("grad_mode", ["autograd", "direct"])
@pytest.mark.parametrize("case", ["c0", "c1", "c2"])
def test_update_matches_the_reference_end_to_end(case, grad_mode, keep):
    z = np.load(os.path.join(GOLDEN, "gradnorm.npz"), allow_pickle=False)
    cc = dict(CASE_CFG[case])
    ckpt = cc.pop("ckpt")
    cfg = gradnorm_cfg(SPEC, **cc)
    cfg.TRAIN.GRADIENT_CHECKPOINTING.ENABLED_GRADNORM_STEPS = ckpt
    model = tiny(cfg=cfg, grad_mode=grad_mode)
    gw = GradientWeighting(TASKS, cfg, "gradnorm", alpha=cc["ALPHA"], keep_step_grads=keep)
    gw.set_model(model)
    names = [str(n) for n in z[f"{case}_param_names"]]
    assert names == [n for n, _ in model.named_parameters()]
    assert [n in gw.backbone_names for n in names] == list(z[f"{case}_backbone"])
    crit = soft_criteria(z)
    model.train()
    for call in range(2):
        x, meta = O.seeded_inputs(SPEC, 4, 64, SEED + 100 + call)
        x, meta = x.cuda(), meta.cuda()
        targets = {t: torch.from_numpy(z[f"target_{call}_{t}"]).cuda() for t in TASKS}
        for p in model.parameters():
            p.grad = None
        O.probe_loss(model(x, meta)).backward()
        before = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        metrics = gw.update_gradnorm_weights_reforward((x, targets, meta), crit, amp_enabled=False, current_step=call)
        want = dict(zip([str(k) for k in z[f"{case}_{call}_metric_keys"]], z[f"{case}_{call}_metrics"]))
        assert set(metrics) == set(want)
        for k, v in want.items():
            rel = 2e-4 if ("/norm/" in k or "/loss/" in k or k.endswith("avg_norm")) else 1e-3
            assert metrics[k] == pytest.approx(v, rel=rel, abs=1e-6), (call, k)
        np.testing.assert_allclose(gw.gradnorm.task_weights.cpu().numpy(), z[f"{case}_{call}_weights"], rtol=1e-3)
        np.testing.assert_allclose(gw.gradnorm.initial_losses.cpu().numpy(), z[f"{case}_{call}_initial_losses"], rtol=2e-4)
        none = [p.grad is None for _, p in model.named_parameters()]
        if keep:
            assert not any(none)
            for n, p in model.named_parameters():
                assert torch.equal(p.grad, before[n]), n
        else:
            assert none == list(z[f"{case}_{call}_grad_none"])
            for n, p in model.named_parameters():
                if p.grad is not None:
                    assert torch.equal(p.grad, before[n]), n


def sm_model(dtype, batch_cfg=None):
    spec = CASES["sm"]
    cfg = gradnorm_cfg(spec, 224)
    model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, O.seeded_state_dict(O.param_shapes(spec), SEED)), strict=True)
    model = model.cuda()
    model.set_compute_dtype(dtype)
    return spec, cfg, model


def test_bf16_sm_norms_close_to_fp32_and_no_host_sync():
    """sm at batch 32: bf16-mode norms within 5e-2 relative of fp32 mode (bf16 operands, 8 mantissa bits, through ~40 layers:
    the step's own gradients agree to a few 1e-3 per element, a norm averages that), and a sync=False update issues no host sync."""
    spec = CASES["sm"]
    B = 32
    g = torch.Generator().manual_seed(SEED + 7)
    x = torch.rand(B, 3, 224, 224, generator=g).cuda()
    meta = (torch.rand(B, spec.meta_width, generator=g) * 2 - 1).cuda()
    targets = {t: torch.randint(0, c, (B,), generator=g).cuda() for t, c in spec.heads}
    crit = {t: TaxonomyAwareLabelSmoothingCE(torch.eye(c) * 0.9 + 0.1 / c).cuda() for t, c in spec.heads}
    res = {}
    for dtype in ("fp32", "bf16"):
        _, cfg, model = sm_model(dtype)
        gw = GradientWeighting([t for t, _ in spec.heads], cfg, "gradnorm")
        gw.set_model(model)
        res[dtype] = gw.update_gradnorm_weights_reforward((x, targets, meta), crit)
        if dtype == "bf16":
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                m = gw.update_gradnorm_weights_reforward((x, targets, meta), crit, sync=False)
            finally:
                torch.cuda.set_sync_debug_mode(0)
            assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in m.values())
            assert float(m["gradnorm/avg_norm"]) == pytest.approx(res["bf16"]["gradnorm/avg_norm"], rel=1e-2)
        del model, gw
        torch.cuda.empty_cache()
    for t, _ in spec.heads:
        assert res["bf16"][f"gradnorm/norm/{t}"] == pytest.approx(res["fp32"][f"gradnorm/norm/{t}"], rel=5e-2)
        assert res["bf16"][f"gradnorm/loss/{t}"] == pytest.approx(res["fp32"][f"gradnorm/loss/{t}"], rel=1e-2)


def test_weighted_loss_with_gradnorm_weighting_equals_static_at_equal_weights():
    g = torch.Generator().manual_seed(3)
    outputs = {t: torch.randn(6, c, generator=g).cuda() for t, c in SPEC.heads}
    targets = {t: torch.randint(0, c, (6,), generator=g).cuda() for t, c in SPEC.heads}
    crit = {t: TaxonomyAwareLabelSmoothingCE(torch.eye(c)).cuda() for t, c in SPEC.heads}
    static = GradientWeighting(TASKS, None, "static")
    gn = GradientWeighting(TASKS, gradnorm_cfg(SPEC), "gradnorm").cuda()
    a_tot, a_comp, a_w = weighted_hierarchical_loss(outputs, targets, crit, static, None, 0, is_validation=True)
    b_tot, b_comp, b_w = weighted_hierarchical_loss(outputs, targets, crit, gn, None, 0, is_validation=True)
    assert float(a_tot) == float(b_tot)
    assert a_comp["weighted_tasks"] == b_comp["weighted_tasks"]
    assert {t: float(v) for t, v in a_w.items()} == {t: float(v) for t, v in b_w.items()}
