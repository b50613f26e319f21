"""Input gradients of the HIP mFormerV1: `images.requires_grad_(True)` / `meta.requires_grad_(True)`, `loss.backward()`.

Parity: x.grad and meta.grad against autograd through the CPU oracle (oracle.mformer_oracle.forward) on the golden cases, relative L2
error, with the bounds of tests/test_gpu_model.py::test_backward_matches_oracle: fp32 2e-3 (its per-parameter bound), bf16 image 10 %
(its per-parameter bound), bf16 metadata 25 % (its bound for the meta_* parameters: one pre-activation of a metadata head that rounds
across zero flips a ReLU mask, and the metadata gradient passes through exactly those masks).  Measured errors are printed.

Consistency (deterministic mode, where equal work means equal bits): asking for input gradients changes no parameter gradient, freezing
parameters changes no input gradient, recompute plans and repeated backwards behave as autograd does."""
import ctypes as C

import pytest
import torch

import linnaeus_amd
from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from linnaeus_amd.inference import input_attribution
from oracle import mformer_oracle as O
from tests.cases import CASES, TinyTree, load_case, make_config, model_state_dict_from_oracle

pytestmark = pytest.mark.gpu
IMG = {"tiny_a": 64, "tiny_b": 96, "tiny_c": 64, "tiny_dp": 64, "sm": 224}


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    linnaeus_amd.set_deterministic(False)


def build(name, spec, sd, dtype):
    kw = {"num_classes": {t: c for t, c in spec.heads}}
    head_type = "Linear"
    if name == "tiny_c":
        head_type = "ConditionalClassifier"
        kw["taxonomy_tree"] = TinyTree({"taxa_L10": {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2}, "taxa_L20": {0: 0, 1: 0, 2: 1}},
                                       [t for t, _ in spec.heads], {t: c for t, c in spec.heads})
    model = build_model(make_config(spec, IMG[name], head_type), **kw)
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype(dtype)
    return model


_ORACLE = {}


def oracle_input_grads(name, golden_dir):
    """(dx, dmeta or None) of the probe loss through the CPU oracle, computed once per case and shared by the dtypes"""
    if name not in _ORACLE:
        spec, z, sd, x, meta, drops = load_case(name, golden_dir)
        xr = x.clone().requires_grad_(True)
        mr = meta.clone().requires_grad_(True) if meta is not None else None
        O.probe_loss(O.forward(sd, spec, xr, mr, drops)).backward()
        _ORACLE[name] = (xr.grad.clone(), mr.grad.clone() if mr is not None else None)
    return _ORACLE[name]


def rel_l2(got, ref):
    return ((got.double().cpu() - ref.double()).norm() / ref.double().norm()).item()


def hip_input_grads(model, x, meta, drops, **fwd_kw):
    xg = x.cuda().requires_grad_(True)
    mg = meta.cuda().requires_grad_(True) if meta is not None else None
    model.train(True)
    model._inject_drop = drops
    O.probe_loss(model(xg, mg, **fwd_kw)).backward()
    return xg, mg


# every tiny case in both dtypes, and one fp32 case at sm (B = 2): the fused stem geometry inside the whole model
PARITY = [(n, d) for n in ("tiny_a", "tiny_b", "tiny_c", "tiny_dp") for d in ("fp32", "bf16")] + [("sm", "fp32")]


@pytest.mark.parametrize("name,dtype", PARITY)
def test_input_grads_match_oracle(name, dtype, golden_dir):
    spec, z, sd, x, meta, drops = load_case(name, golden_dir)
    model = build(name, spec, sd, dtype)
    fused = bool(L.lib().lnx_stem_dgrad_ok(model._dtype_code, 3, IMG[name], IMG[name], spec.conv_dims[0]))
    assert fused == (name == "sm")  # sm: lnx_stem_dgrad; the tiny cases (Cout = 32): lnx_gemm_nt + lnx_col2im_stem
    xg, mg = hip_input_grads(model, x, meta, drops)
    rx, rm = oracle_input_grads(name, golden_dir)
    assert xg.grad is not None and xg.grad.shape == x.shape and xg.grad.dtype == torch.float32
    ex = rel_l2(xg.grad, rx)
    print(f"[{name}/{dtype}] image gradient: relative L2 error vs oracle {ex:.3e}")
    assert ex <= (2e-3 if dtype == "fp32" else 0.10)
    if meta is not None:
        assert mg.grad is not None and mg.grad.shape == meta.shape
        em = rel_l2(mg.grad, rm)
        print(f"[{name}/{dtype}] metadata gradient: relative L2 error vs oracle {em:.3e}")
        assert em <= (2e-3 if dtype == "fp32" else 0.25)
    # the parameters still get their gradients from the same backward
    assert all(p_.grad is not None for p_ in model.parameters())


class Det:
    """tiny_b (three metadata components, two blocks in stages 0 and 2) in deterministic mode"""

    def __init__(self, golden_dir, dtype="fp32", name="tiny_b"):
        self.spec, _, self.sd, self.x, self.meta, self.drops = load_case(name, golden_dir)
        self.model = build(name, self.spec, self.sd, dtype)
        self.model.set_deterministic(True)

    def step(self, want_x=True, want_meta=True, **fwd_kw):
        m = self.model
        m.train(True)
        m._inject_drop = self.drops
        m.zero_grad(set_to_none=True)
        xg = self.x.cuda().requires_grad_(want_x)
        mg = self.meta.cuda().requires_grad_(want_meta)
        O.probe_loss(m(xg, mg, **fwd_kw)).backward()
        torch.cuda.synchronize()
        return xg.grad, mg.grad, {k: p_.grad.clone() for k, p_ in m.named_parameters() if p_.grad is not None}


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_parameter_gradients_do_not_depend_on_the_input_flags(dtype, golden_dir):
    d = Det(golden_dir, dtype)
    _, _, plain = d.step(False, False)
    dx, dm, both = d.step(True, True)
    assert dx is not None and dm is not None
    assert plain.keys() == both.keys() and len(plain) == len(list(d.model.parameters()))
    assert not [k for k in plain if not torch.equal(plain[k], both[k])]
    dx_only, none_m, _ = d.step(True, False)
    none_x, dm_only, _ = d.step(False, True)
    assert none_m is None and none_x is None
    assert torch.equal(dx_only, dx) and torch.equal(dm_only, dm)
    # a second identical step: the same bits (no atomics, a fixed order for the two contributions of a metadata component)
    dx2, dm2, _ = d.step(True, True)
    assert torch.equal(dx2, dx) and torch.equal(dm2, dm)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frozen_parameters_change_no_input_gradient(dtype, golden_dir):
    d = Det(golden_dir, dtype)
    dx, dm, full = d.step(True, True)
    for p_ in d.model.parameters():
        p_.requires_grad_(False)
    fx, fm, none = d.step(True, True)
    assert torch.equal(fx, dx) and torch.equal(fm, dm)
    assert none == {} and all(p_.grad is None for p_ in d.model.parameters())
    units = d.model.plan_units()["units"]
    assert units[L.lib().lnx_plan_first_trained_unit(d.model._active["handle"])] == "stem"
    # only the metadata differentiated, nothing trained: the backward stops behind tokens_1
    _, fm2, _ = d.step(False, True)
    assert torch.equal(fm2, dm)
    assert units[L.lib().lnx_plan_first_trained_unit(d.model._active["handle"])] == "tokens_1"
    # a frozen prefix: the trainable parameters' gradients with and without the image gradient
    d.model.freeze_through("stages.2.0")
    _, _, cut = d.step(False, False)
    assert units[L.lib().lnx_plan_first_trained_unit(d.model._active["handle"])] == "stages.2.0"
    cx, _, cut_x = d.step(True, False)
    assert torch.equal(cx, dx)
    trainable = {k for k, p_ in d.model.named_parameters() if p_.requires_grad}
    assert cut.keys() == cut_x.keys() == trainable and 0 < len(trainable) < len(full)
    assert not [k for k in cut if not torch.equal(cut[k], cut_x[k])]


def test_recompute_plan_gives_the_same_bits(golden_dir):
    d = Det(golden_dir, "bf16")
    dx, dm, _ = d.step(True, True)
    rx, rm, _ = d.step(True, True, force_checkpointing=True)
    assert torch.equal(rx, dx) and torch.equal(rm, dm)


def test_launch_by_launch_heads_give_the_same_metadata_gradient(golden_dir, monkeypatch):
    d = Det(golden_dir, "fp32")
    _, dm, _ = d.step(True, True)
    monkeypatch.setenv("LNX_META_CHAIN", "0")  # read when a plan is created
    d.model.release_plans()
    _, dm0, _ = d.step(True, True)
    monkeypatch.delenv("LNX_META_CHAIN")
    d.model.release_plans()
    err = rel_l2(dm0, dm.cpu())
    print(f"[tiny_b/fp32] metadata gradient, launch-by-launch heads vs one-launch chain: relative L2 difference {err:.3e}")
    assert err <= 2e-3  # the fp32 bound of the parity test: two fp32 routes to the same sums
    rm = oracle_input_grads("tiny_b", golden_dir)[1]
    assert rel_l2(dm0, rm) <= 2e-3


def test_autograd_grad_two_backwards_and_features(golden_dir):
    d = Det(golden_dir, "fp32")
    dx, dm, _ = d.step(True, True)
    m = d.model
    xg, mg = d.x.cuda().requires_grad_(True), d.meta.cuda().requires_grad_(True)
    gx, gm = torch.autograd.grad(O.probe_loss(m(xg, mg)), [xg, mg])
    assert torch.equal(gx, dx) and torch.equal(gm, dm)
    assert xg.grad is None and all(p_.grad is not None for p_ in m.parameters())  # (.grad of the step before; autograd.grad touches none)
    # two forward / backward passes accumulate into the leaf as autograd does
    for _ in range(2):
        O.probe_loss(m(xg, mg)).backward()
    assert torch.equal(xg.grad, 2 * dx) and torch.equal(mg.grad, 2 * dm)
    assert xg.grad.data_ptr() != m._active["ws"].data_ptr()
    # forward_features: the same path with a gradient on the features only
    xf, mf = d.x.cuda().requires_grad_(True), d.meta.cuda().requires_grad_(True)
    m.forward_features(xf, mf).square().sum().backward()
    assert xf.grad is not None and mf.grad is not None and xf.grad.abs().max() > 0 and mf.grad.abs().max() > 0
    # no graph under no_grad, input flags or not
    with torch.no_grad():
        out = m(xg, mg)
    assert not any(v.requires_grad for v in out.values())


def test_eval_mode_and_set_after_bind(golden_dir):
    """model.eval() with x.requires_grad: a training plan with DropPath and dropout off -- the logits are those of the inference plan"""
    spec, z, sd, x, meta, drops = load_case("tiny_dp", golden_dir)
    model = build("tiny_dp", spec, sd, "fp32")
    model.eval()
    with torch.no_grad():
        want = {k: v.clone() for k, v in model(x.cuda(), meta.cuda()).items()}
    xg = x.cuda().requires_grad_(True)
    out = model(xg, meta.cuda())
    for k in want:
        assert torch.equal(out[k], want[k]), k
    O.probe_loss(out).backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all() and xg.grad.abs().max() > 0
    lib = L.lib()
    h = model._active["handle"]
    assert lib.lnx_plan_input_grads(h) == 1
    assert lib.lnx_plan_set_input_grads(h, 1, 1) != 0  # the plan is bound
    assert "already bound" in lib.lnx_last_error().decode()


def test_input_attribution(golden_dir):
    d = Det(golden_dir, "fp32")
    m = d.model
    x, meta = d.x.cuda(), d.meta.cuda()
    task = d.spec.heads[0][0]
    att = input_attribution(m, x, meta, task)
    B, _, H, W = x.shape
    assert att["image"].shape == (B, H, W)
    assert list(att["meta"]) == [n for n, _ in d.spec.meta] and all(v.shape == (B,) for v in att["meta"].values())
    assert m.training  # the mode is put back
    # by hand: eval mode, the predicted class logit of every sample as the seed
    m.eval()
    xg, mg = x.clone().requires_grad_(True), meta.clone().requires_grad_(True)
    logits = m(xg, mg)[task].float()
    logits.gather(1, logits.argmax(-1, keepdim=True)).sum().backward()
    m.train(True)
    assert torch.equal(att["image"], xg.grad.abs().amax(1))
    off = 0
    for n, dim in d.spec.meta:
        assert torch.equal(att["meta"][n], mg.grad[:, off: off + dim].norm(dim=1)), n
        off += dim
    gxi = input_attribution(m, x, meta, task, class_index=1, kind="grad_x_input")
    assert gxi["image"].shape == (B, H, W)
    with pytest.raises(ValueError):
        input_attribution(m, x, meta, task, kind="other")


def test_per_task_backward_leaves_input_gradients_alone(golden_dir):
    """lnx_plan_backward_into (GradNorm's per-task backward) never writes dx / dmeta, even on a plan made for them with both bound; the
    ordinary backward of the same forward then does"""
    spec, z, sd, x, meta, drops = load_case("tiny_a", golden_dir)
    model = build("tiny_a", spec, sd, "fp32")
    model.train(True)
    xg, mg = x.cuda().requires_grad_(True), meta.cuda().requires_grad_(True)
    out = model(xg, mg)
    st, lib = model._active, L.lib()
    assert lib.lnx_plan_input_grads(st["handle"]) == 3
    dx, dm = torch.full_like(xg, float("nan")), torch.full_like(mg, float("nan"))
    L.check(lib.lnx_plan_bind_input_grads(st["handle"], C.c_void_p(dx.data_ptr()), C.c_void_p(dm.data_ptr())), "lnx_plan_bind_input_grads")
    scratch = torch.zeros_like(model._grad_arena)
    base = model._grad_arena.data_ptr()
    ptrs = (C.c_void_p * st["n"])(*[scratch.data_ptr() + (v.data_ptr() - base) for v in model._grad_views])
    dl = torch.ones(max(st["logits_numel"], 1), device="cuda")
    L.check(lib.lnx_plan_backward_into(st["handle"], C.c_void_p(dl.data_ptr()), None, ptrs, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "lnx_plan_backward_into")
    torch.cuda.synchronize()
    assert torch.isnan(dx).all() and torch.isnan(dm).all()
    assert scratch.abs().sum().item() > 0
    O.probe_loss(out).backward()
    rx, rm = oracle_input_grads("tiny_a", golden_dir)
    assert rel_l2(xg.grad, rx) <= 2e-3 and rel_l2(mg.grad, rm) <= 2e-3
    assert torch.isnan(dx).all() and torch.isnan(dm).all()  # (the autograd backward binds fresh tensors of its own)
