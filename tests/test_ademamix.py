"""FusedAdEMAMix (linnaeus_amd/optim.py, ademamix_kernel in csrc/optim.hip): the reference's AdEMAMix
(linnaeus/optimizers/ademamix.py) as one multi-tensor HIP launch per step, three with the global-norm clip.

CPU: the ctypes mirror of lnx_ademamix_hyper, constructor defaults and validation, and the reference's state layout.
GPU: the reference's own steps (tests/golden/ademamix.npz, tests/golden/gen/make_golden_ademamix.py), a resume from its
step-3 state, a float64 restatement of the update with clipping and unaligned arena views, per-parameter step counts,
bit-reproducibility, and the model's direct-mode gradient arena.

Tolerance: the fixture and the float64 restatement agree with the kernel to fp32 rounding.  Every step rounds p once
more in fp32 (half an ulp, 6e-8 relative at |p| ~ 1) and the update term, ~lr in size, carries a few ulps of its own
relative error; over six steps that stays well under rtol 2e-6 / atol 2e-7, the bound tests/test_optim.py uses for
FusedAdamW against torch.optim.AdamW.  The EMA states are compared with the same rtol, but their atol scales with the
gradients: m1 and m3 are sums of terms of size |g| that can cancel (b1 m1 + (1-b1) g near zero), so their rounding error
is a few fp32 ulps of the largest term, not of the result -- atol = 8 ulps (2^-21) of max|g| (of max g^2 for v).
"""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2e-6, 2e-7
KEYS = ("exp_avg", "exp_avg_sq", "exp_avg_slow")


def assert_state_close(got, want, gmax, label):
    """got / want: {state key: tensor}; gmax: largest |gradient| this parameter has seen (see the module docstring)"""
    for k in KEYS:
        atol = 2.0 ** -21 * (gmax * gmax if k == "exp_avg_sq" else gmax)
        torch.testing.assert_close(got[k].double().cpu(), want[k].double().cpu(), rtol=RTOL, atol=atol, msg=lambda m: f"{label} {k}: {m}")


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_hyper_mirror_has_the_size_the_c_compiler_gives(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n'
                   '    printf("%zu %zu\\n", sizeof(lnx_ademamix_hyper), offsetof(lnx_ademamix_hyper, omb3));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    size, off = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(L.AdEMAMixHyper)
    assert off == L.AdEMAMixHyper.omb3.offset
    assert "lnx_ademamix_step" in L.EXPORTS


def test_step_entry_validates_on_the_host():
    """slot count, bias corrections and null tables are refused before any launch (the pointers are never dereferenced)"""
    lib = L.lib()
    fake = C.c_void_p(0x1000)
    h = L.AdEMAMixHyper()
    h.ngroups = 1
    h.bias_c1[0], h.bias_c2[0] = 0.1, 0.001
    assert lib.lnx_ademamix_step(fake, None, 1, 1, C.byref(h), None, 0.0, None) != 0
    assert b"lnx_ademamix_step" in lib.lnx_last_error()
    h.ngroups = L.ADAMW_MAX_GROUPS + 1
    assert lib.lnx_ademamix_step(fake, fake, 1, 1, C.byref(h), None, 0.0, None) != 0
    assert b"ngroups" in lib.lnx_last_error()
    h.ngroups = 1
    h.bias_c1[0] = 0.0
    assert lib.lnx_ademamix_step(fake, fake, 1, 1, C.byref(h), None, 0.0, None) != 0
    assert b"bias corrections" in lib.lnx_last_error()


def test_constructor_defaults_and_group_keys():
    from linnaeus_amd.optim import FusedAdEMAMix

    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2))]
    opt = FusedAdEMAMix([{"params": ps[:1]}, {"params": ps[1:], "lr": 1e-2, "T_alpha_beta3": 100}])
    assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0, alpha=5.0, T_alpha_beta3=None)
    for g in opt.param_groups:
        assert {"lr", "betas", "eps", "weight_decay", "alpha", "T_alpha_beta3"} <= set(g)
    assert opt.param_groups[1]["T_alpha_beta3"] == 100 and opt.param_groups[0]["T_alpha_beta3"] is None
    assert opt.max_grad_norm is None


@pytest.mark.parametrize("kw", [
    dict(lr=-1e-3), dict(eps=-1.0), dict(weight_decay=-0.1),
    dict(betas=(0.9, 0.999)), dict(betas=(0.9, 0.999, 1.0)), dict(betas=(-0.1, 0.999, 0.9999)),
    # the reference accepts these and then fails inside its first step (division by zero / log(0)):
    dict(T_alpha_beta3=0), dict(T_alpha_beta3=-5), dict(T_alpha_beta3=10, betas=(0.0, 0.999, 0.9999)), dict(T_alpha_beta3=10, betas=(0.9, 0.999, 0.0)),
])
def test_constructor_refuses(kw):
    from linnaeus_amd.optim import FusedAdEMAMix

    with pytest.raises(ValueError):
        FusedAdEMAMix([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_constructor_refuses_a_bad_group():
    from linnaeus_amd.optim import FusedAdEMAMix

    with pytest.raises(ValueError):
        FusedAdEMAMix([{"params": [torch.nn.Parameter(torch.zeros(3))], "T_alpha_beta3": 10, "betas": (0.0, 0.9, 0.99)}])


def test_zero_betas_without_schedule_are_accepted():
    from linnaeus_amd.optim import FusedAdEMAMix

    FusedAdEMAMix([torch.nn.Parameter(torch.zeros(3))], betas=(0.0, 0.0, 0.0))


def test_schedule_values():
    from linnaeus_amd.optim import ademamix_schedule

    assert ademamix_schedule(7, 5.0, 0.9, 0.9999, None) == (5.0, 0.9999)
    a, b3 = ademamix_schedule(1, 2.0, 0.8, 0.999, 4)
    assert a == 0.5
    # log-interpolation between beta1 (step 0) and beta3 (step T), in the half-life sense
    want = math.exp(math.log(0.8) * math.log(0.999) / (0.75 * math.log(0.999) + 0.25 * math.log(0.8)))
    assert b3 == want and 0.8 < b3 < 0.999
    assert ademamix_schedule(4, 2.0, 0.8, 0.999, 4) == pytest.approx((2.0, 0.999), rel=1e-12)
    assert ademamix_schedule(9, 2.0, 0.8, 0.999, 4) == (2.0, 0.999)  # capped past T


def test_load_state_dict_of_the_reference_layout():
    """a state dict shaped as the reference AdEMAMix writes it (int or tensor step, three EMA buffers per parameter)"""
    from linnaeus_amd.optim import FusedAdEMAMix

    ps = [torch.nn.Parameter(torch.zeros(4)), torch.nn.Parameter(torch.zeros(2, 3))]
    opt = FusedAdEMAMix(ps, lr=2e-3, T_alpha_beta3=50)
    sd = {
        "state": {
            0: {"step": 7, "exp_avg": torch.full((4,), 0.1), "exp_avg_sq": torch.full((4,), 0.2), "exp_avg_slow": torch.full((4,), 0.3)},
            1: {"step": torch.tensor(7.0), "exp_avg": torch.ones(2, 3), "exp_avg_sq": torch.ones(2, 3), "exp_avg_slow": torch.ones(2, 3)},
        },
        "param_groups": [{"lr": 5e-4, "betas": (0.9, 0.999, 0.9999), "eps": 1e-8, "weight_decay": 0.05, "alpha": 5.0, "T_alpha_beta3": 50,
                          "params": [0, 1]}],
    }
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == 5e-4 and opt.param_groups[0]["weight_decay"] == 0.05
    assert set(opt.state[ps[0]]) == {"step", *KEYS}
    assert torch.equal(opt.state[ps[0]]["exp_avg_slow"], torch.full((4,), 0.3))
    back = opt.state_dict()
    assert set(back["state"][1]) == {"step", *KEYS} and int(back["state"][1]["step"]) == 7


def test_cpu_parameters_are_refused():
    from linnaeus_amd.optim import FusedAdEMAMix

    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(L.LnxError):
        FusedAdEMAMix([p]).step()


# ----------------------------------------------------------------------------------------- float64 restatement (GPU tests)
def ref_step(p, g, st, group, coef=1.0):
    """one AdEMAMix update of one parameter in float64, written from the update rule (weight decay decoupled and first;
    the slow EMA divided by bias_c1 as well).  p: float64 tensor updated in place; st: float64 state dict, step included."""
    b1, b2, b3 = group["betas"]
    lr, wd, eps, alpha, T = group["lr"], group["weight_decay"], group["eps"], group["alpha"], group["T_alpha_beta3"]
    st["step"] += 1
    t = st["step"]
    alpha_t, b3t = alpha, b3
    if T is not None:
        alpha_t = min(t * alpha / T, alpha)
        b3t = min(math.exp(math.log(b1) * math.log(b3) / ((1 - t / T) * math.log(b3) + (t / T) * math.log(b1))), b3)
    g = g.double() * coef
    p.mul_(1 - lr * wd)
    st["exp_avg"].mul_(b1).add_((1 - b1) * g)
    st["exp_avg_sq"].mul_(b2).add_((1 - b2) * g * g)
    st["exp_avg_slow"].mul_(b3t).add_((1 - b3t) * g)
    denom = st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** t) + eps
    p.sub_(lr / (1 - b1 ** t) * (st["exp_avg"] + alpha_t * st["exp_avg_slow"]) / denom)


def ref_init(p):
    return {"step": 0, **{k: torch.zeros_like(p, dtype=torch.float64) for k in KEYS}}


def clip_coef(grads, max_norm):
    if max_norm is None:
        return 1.0, None
    n = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))
    return min(1.0, max_norm / (n + 1e-6)), n


def fixture_groups(params, z):
    return [{"params": params[:3], "lr": float(z["group0_lr"][0]), "weight_decay": 0.05},
            {"params": params[3:], "lr": 1e-2, "weight_decay": 0.0, "betas": (0.8, 0.95, 0.999), "alpha": 2.0, "T_alpha_beta3": 4}]


def fixture_optimizer(z):
    from linnaeus_amd.optim import FusedAdEMAMix

    params = [torch.nn.Parameter(torch.from_numpy(z[f"p{i}_init"]).cuda()) for i in range(6)]
    return params, FusedAdEMAMix(fixture_groups(params, z), lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0, alpha=5.0)


def replay(z, params, opt, steps):
    for s in steps:
        opt.param_groups[0]["lr"] = float(z["group0_lr"][s])
        for i, p in enumerate(params):
            p.grad = torch.from_numpy(z[f"p{i}_grad{s}"]).cuda()
        opt.step()


@pytest.mark.gpu
def test_replays_the_reference_fixture(golden_dir):
    z = np.load(f"{golden_dir}/ademamix.npz")
    params, opt = fixture_optimizer(z)
    for s in range(6):
        replay(z, params, opt, [s])
        for i, p in enumerate(params):
            torch.testing.assert_close(p.detach().cpu(), torch.from_numpy(z[f"p{i}_after{s}"]), rtol=RTOL, atol=ATOL, msg=lambda m: f"p{i} after step {s + 1}: {m}")
    for i, p in enumerate(params):
        assert opt.state[p]["step"] == int(z[f"p{i}_step_s6"]) == 6
        gmax = max(float(np.abs(z[f"p{i}_grad{s}"]).max()) for s in range(6))
        assert_state_close(opt.state[p], {k: torch.from_numpy(z[f"p{i}_{k}_s6"]) for k in KEYS}, gmax, f"p{i}")


@pytest.mark.gpu
def test_resumes_from_the_reference_step_3_state(golden_dir):
    """a checkpoint the reference wrote after step 3 (its state_dict layout), continued by FusedAdEMAMix to step 6"""
    z = np.load(f"{golden_dir}/ademamix.npz")
    params, opt = fixture_optimizer(z)
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(torch.from_numpy(z[f"p{i}_after2"]))
    sd = {"state": {i: {"step": torch.tensor(float(z[f"p{i}_step_s3"])), **{k: torch.from_numpy(z[f"p{i}_{k}_s3"]) for k in KEYS}} for i in range(6)},
          "param_groups": [{k: v for k, v in g.items() if k != "params"} | {"params": list(range(3 * gi, 3 * gi + 3))}
                           for gi, g in enumerate(opt.param_groups)]}
    opt.load_state_dict(sd)
    replay(z, params, opt, range(3, 6))
    for i, p in enumerate(params):
        torch.testing.assert_close(p.detach().cpu(), torch.from_numpy(z[f"p{i}_after5"]), rtol=RTOL, atol=ATOL, msg=lambda m: f"p{i}: {m}")
        assert opt.state[p]["step"] == 6


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [None, 0.5, 1e6])
def test_matches_float64_with_clipping_and_unaligned_views(clip):
    """parameters at odd element offsets of one flat buffer (no 16-byte alignment for p, and -- with state and gradients
    carved the same way -- for g, m1, v and m3), sizes 1 and 4096 k + 1, next to ordinary aligned tensors"""
    from linnaeus_amd.optim import FusedAdEMAMix

    gen = torch.Generator().manual_seed(11)
    sizes = [1, 4097, 3 * 4096 + 1, 37]
    flat = torch.randn(1 + sum(sizes) + len(sizes), generator=gen).cuda()
    views, off = [], 1
    for n in sizes:
        views.append(flat[off: off + n])
        off += n + 1  # odd offsets: 1, 4099, ...
    aligned = [torch.randn(s, generator=gen).cuda() for s in ((4096 * 2 + 1,), (64, 33))]
    params = [torch.nn.Parameter(t) for t in views] + [torch.nn.Parameter(t) for t in aligned]
    assert any(p.data_ptr() % 16 for p in params)
    groups = [{"params": params[:3], "lr": 3e-3, "weight_decay": 0.05},
              {"params": params[3:], "lr": 1e-2, "betas": (0.8, 0.95, 0.999), "alpha": 2.0, "T_alpha_beta3": 3}]
    opt = FusedAdEMAMix(groups, max_grad_norm=clip)
    ref_p = [p.detach().double().clone() for p in params]
    ref_st = [ref_init(p) for p in params]
    gflat = torch.empty(flat.numel(), device="cuda")
    gmax = [0.0] * len(params)
    for step in range(5):
        # gradients as unaligned views of one buffer too
        gflat.copy_(torch.randn(flat.numel(), generator=gen) * (0.1 + step))
        off = 1
        for p, n in zip(params[:4], sizes):
            p.grad = gflat[off: off + n]
            off += n + 1
        for p in params[4:]:
            p.grad = torch.randn(p.shape, generator=gen).cuda() * (0.1 + step)
        if step == 0:
            for p in params[:4]:  # state tensors carved at odd offsets as well: all five pointers unaligned
                st = opt.state[p]
                st["step"] = 0
                for k in KEYS:
                    buf = torch.zeros(p.numel() + 1, device="cuda")
                    st[k] = buf[1:]
        gmax = [max(m, float(p.grad.abs().max())) for m, p in zip(gmax, params)]
        coef, norm = clip_coef([p.grad for p in params], clip)
        if clip is not None:  # torch's clip on stand-in tensors carrying copies of the gradients
            stand_in = [torch.zeros_like(p).requires_grad_(True) for p in params]
            for q, p in zip(stand_in, params):
                q.grad = p.grad.clone()
            want = torch.nn.utils.clip_grad_norm_(stand_in, clip)
        opt.step()
        if clip is not None:
            assert abs(float(opt.grad_norm()) - norm) <= 1e-5 * norm
            torch.testing.assert_close(opt.grad_norm(), want, rtol=1e-5, atol=1e-6)
        for gi, group in enumerate(groups):
            for p in group["params"]:
                j = next(i for i, q in enumerate(params) if q is p)
                ref_step(ref_p[j], p.grad, ref_st[j], opt.param_groups[gi], coef)
        for j, p in enumerate(params):
            torch.testing.assert_close(p.detach().double(), ref_p[j], rtol=RTOL, atol=ATOL, msg=lambda m: f"param {j} step {step + 1}: {m}")
    for j, p in enumerate(params):
        assert_state_close(opt.state[p], ref_st[j], gmax[j], f"param {j}")


@pytest.mark.gpu
def test_parameters_on_different_step_counts_get_their_own_schedule():
    """a parameter without a gradient on some steps lags the others: its bias corrections, alpha_t and beta3_t follow its
    own step count (one hyper-parameter slot per (group, step) pair); more than 16 such slots are refused"""
    from linnaeus_amd.optim import FusedAdEMAMix

    gen = torch.Generator().manual_seed(5)
    params = [torch.nn.Parameter(torch.randn(257, generator=gen).cuda()) for _ in range(3)]
    opt = FusedAdEMAMix(params, lr=1e-2, weight_decay=0.01, alpha=3.0, T_alpha_beta3=4)
    ref_p = [p.detach().double().clone() for p in params]
    ref_st = [ref_init(p) for p in params]
    for step in range(6):
        for i, p in enumerate(params):
            p.grad = None if (i == 1 and step in (1, 2)) else torch.randn(p.shape, generator=gen).cuda()
        opt.step()
        for j, p in enumerate(params):
            if p.grad is not None:
                ref_step(ref_p[j], p.grad, ref_st[j], opt.param_groups[0])
            torch.testing.assert_close(p.detach().double(), ref_p[j], rtol=RTOL, atol=ATOL, msg=lambda m: f"param {j} step {step + 1}: {m}")
    assert opt.state[params[1]]["step"] == 4 and opt.state[params[0]]["step"] == 6

    many = [torch.nn.Parameter(torch.zeros(5, device="cuda")) for _ in range(L.ADAMW_MAX_GROUPS + 1)]
    opt = FusedAdEMAMix(many)
    for i, p in enumerate(many):
        p.grad = torch.ones(5, device="cuda")
        opt.state[p].update(step=i, **{k: torch.zeros(5, device="cuda") for k in KEYS})
    with pytest.raises(L.LnxError, match="step count"):
        opt.step()


@pytest.mark.gpu
def test_two_instances_take_bit_identical_steps():
    """data-parallel replicas hold identical gradients and must stay bit-identical: clip norm in a fixed order, no atomics"""
    from linnaeus_amd.optim import FusedAdEMAMix

    gen = torch.Generator().manual_seed(9)
    init = [torch.randn(n, generator=gen) for n in (2_000_003, 777, 4096 * 50 + 1)]
    pa = [torch.nn.Parameter(t.cuda()) for t in init]
    pb = [torch.nn.Parameter(t.cuda()) for t in init]
    oa, ob = (FusedAdEMAMix(ps, lr=1e-3, weight_decay=0.05, T_alpha_beta3=3, max_grad_norm=1.0) for ps in (pa, pb))
    for step in range(4):
        for a, b in zip(pa, pb):
            g = torch.randn(a.shape, generator=gen).cuda() * 1e-2
            a.grad, b.grad = g.clone(), g.clone()
        oa.step()
        ob.step()
        assert torch.equal(oa.grad_norm(), ob.grad_norm())
        for a, b in zip(pa, pb):
            assert torch.equal(a, b), step
            for k in KEYS:
                assert torch.equal(oa.state[a][k], ob.state[b][k]), (step, k)


@pytest.mark.gpu
def test_model_steps_on_the_direct_gradient_arena(golden_dir):
    """tiny_a in grad_mode "direct" (gradients are views into one flat arena): three steps match the float64 restatement fed
    copies of the same arena gradients, and the loss falls on a fixed batch"""
    from linnaeus_amd.loss import multitask_cross_entropy
    from linnaeus_amd.optim import FusedAdEMAMix
    from tests.cases import load_train_step
    from tests.test_gpu_model import build

    spec, z, sd, x, meta, targets, weights = load_train_step(golden_dir)
    model = build("tiny_a", spec, sd, "fp32")
    model.train()
    model.grad_mode = "direct"
    xg, mg = x.cuda(), meta.cuda()
    tg = {t: v.cuda() for t, v in targets.items()}
    params = [p for p in model.parameters() if p.requires_grad]
    group = dict(lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0.05, alpha=5.0, T_alpha_beta3=10)
    opt = FusedAdEMAMix(params, max_grad_norm=1.0, **group)
    ref_p = [p.detach().double().clone() for p in params]
    ref_st = [ref_init(p) for p in params]
    losses = []
    for s in range(6):
        model.zero_grad(set_to_none=True)
        loss = multitask_cross_entropy(model(xg, mg), tg, weights)
        loss.backward()
        losses.append(loss.item())
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        coef, _ = clip_coef([g for g in grads if g is not None], 1.0)
        opt.step()
        if s < 3:
            for j, p in enumerate(params):
                if grads[j] is not None:
                    ref_step(ref_p[j], grads[j], ref_st[j], opt.param_groups[0], coef)
                torch.testing.assert_close(p.detach().double(), ref_p[j], rtol=RTOL, atol=ATOL, msg=lambda m: f"param {j} step {s + 1}: {m}")
            ref_p = [p.detach().double().clone() for p in params]  # next step starts from the model's own fp32 values
    print(f"[ademamix/model] losses {['%.4f' % v for v in losses]}")
    assert losses[-1] < losses[0]
