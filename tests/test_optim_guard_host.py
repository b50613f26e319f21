"""The non-finite guard without a GPU: the restatement of tests/optim_guard_ref.py inside torch.amp.GradScaler("cpu") against a skip
written out by hand, the GradScaler protocol of the fused optimizers (an instance property that follows `nonfinite_guard`, a `step`
without a `grad_scaler` parameter), the ctypes mirrors of the new structs, and the host-side argument checks of the new entry points."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import pytest
import torch

from linnaeus_amd import _lib as L
from tests.optim_guard_ref import GuardRef, run

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {
    "adamw": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05),
    "ademamix": dict(lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0.05, alpha=5.0, T_alpha_beta3=10),
    "sgd": dict(lr=0.01, momentum=0.9, dampening=0.0, nesterov=True, weight_decay=0.05),
    "sgd_damp": dict(lr=0.01, momentum=0.9, dampening=0.1, nesterov=False, weight_decay=0.05),
    "muon": dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5),
}
SHAPES = [(5, 8), (16, 3)]


def make(name, seed=1):
    kind = name.split("_")[0]
    gen = torch.Generator().manual_seed(seed)
    dtype = torch.float64 if kind == "ademamix" else torch.float32
    params = [torch.nn.Parameter((torch.randn(*s, generator=gen) * 0.1).to(dtype)) for s in SHAPES]
    return GuardRef(kind, params, GROUPS[name]), params


def grad_sequence(poison, at, steps=5, seed=2):
    gen = torch.Generator().manual_seed(seed)
    seq = [[torch.randn(*s, generator=gen) for s in SHAPES] for _ in range(steps)]
    for s in at:
        seq[s][1][3, 1] = poison
    return seq


@pytest.mark.parametrize("at", [(0,), (2,), (1, 2)], ids=["first", "third", "second+third"])
@pytest.mark.parametrize("poison", [float("inf"), float("-inf"), float("nan")], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("name", list(GROUPS))
def test_restatement_inside_gradscaler_equals_the_skip_written_by_hand(name, poison, at):
    """torch.amp.GradScaler("cpu") decides the skip from the gradients (scale 2^16, halved after every skipped step: powers of two,
    so unscaling is exact); the restatement is told which steps are poisoned.  Both must leave the same bits -- once the host-side
    bookkeeping of the guard, `skip()`, is applied to the scaler's run as well (torch's own skipped step does nothing at all)."""
    seq = grad_sequence(poison, at)
    by_hand, hand_params = make(name)
    run(by_hand, seq, poisoned=at)
    inside, params = make(name)
    scaler = torch.amp.GradScaler("cpu", init_scale=2.0 ** 16)
    for s, grads in enumerate(seq):
        for p in params:
            p.grad = None
        scaler.scale(sum((p * g.to(p.dtype)).sum() for p, g in zip(params, grads))).backward()  # d/dp = g * scale
        scale = scaler.get_scale()
        assert scale == 2.0 ** (16 - sum(1 for a in at if a < s))
        for p, g in zip(params, grads):
            assert torch.equal(p.grad.isfinite(), g.isfinite()) and torch.equal(p.grad[g.isfinite()], (g * scale).to(p.dtype)[g.isfinite()])
        before = [p.detach().clone() for p in params]
        scaler.step(inside)
        scaler.update()
        if s in at:
            assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
            for p, g in zip(params, grads):
                p.grad = g.to(p.dtype)
            inside.skip()
    for p, q in zip(params, hand_params):
        assert torch.equal(p.detach(), q.detach()), name
        a, b = inside.state_of(p), by_hand.state_of(q)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), (name, k)
        if "step" in a:
            assert int(a["step"]) == len(seq)  # attempted steps


def test_a_skip_differs_from_leaving_the_step_out_only_where_the_docs_say():
    """Muon, and SGD at dampening 0, equal the run that never saw the poisoned step; AdamW and AdEMAMix (bias correction by attempted
    steps) and SGD with dampening whose buffer is created on the skipped step do not."""
    for name, same in [("muon", True), ("sgd", True), ("sgd_damp", False), ("adamw", False), ("ademamix", False)]:
        seq = grad_sequence(float("inf"), (0,))
        a, pa = make(name)
        run(a, seq, poisoned=(0,))
        b, pb = make(name)
        run(b, seq[1:])
        assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(pa, pb)) == same, name
    # a buffer that exists is not touched: with dampening, a skip at a later step is the step left out
    seq = grad_sequence(float("nan"), (2,))
    a, pa = make("sgd_damp")
    run(a, seq, poisoned=(2,))
    b, pb = make("sgd_damp")
    run(b, seq[:2] + seq[3:])
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(pa, pb))


# ------------------------------------------------------------------------------------------------------------------ protocol
def fused_classes():
    from linnaeus_amd import optim as M

    w = lambda: [torch.nn.Parameter(torch.zeros(4, 4))]  # noqa: E731
    return M, [lambda **kw: M.FusedAdamW(w(), **kw), lambda **kw: M.FusedAdEMAMix(w(), **kw), lambda **kw: M.FusedSGD(w(), lr=0.1, **kw),
               lambda **kw: M.FusedMuon(w(), **kw), lambda **kw: M.FusedMultiOptimizer({"A": M.FusedAdamW(w()), "M": M.FusedMuon(w())}, **kw)]


def test_amp_scaling_property_follows_the_constructor_argument():
    M, makers = fused_classes()
    for mk in makers:
        off, on, default = mk(nonfinite_guard=False), mk(nonfinite_guard=True), mk()
        assert on._step_supports_amp_scaling is True and on.nonfinite_guard is True
        assert off._step_supports_amp_scaling is False and default._step_supports_amp_scaling is False and default.nonfinite_guard is False
        assert isinstance(getattr(type(on), "_step_supports_amp_scaling"), property)  # per instance, not a class constant
        assert "grad_scaler" not in inspect.signature(on.step).parameters
        assert list(inspect.signature(on.step).parameters) == ["closure"]
        # read-outs exist and say nothing before a step / without the guard
        assert on.skipped_steps() is None and on.last_step_skipped() is None and off.skipped_steps() is None and on.grad_norm() is None


def test_multi_optimizer_refusals_under_the_guard():
    M, _ = fused_classes()
    w = lambda: [torch.nn.Parameter(torch.zeros(4, 4))]  # noqa: E731
    with pytest.raises(ValueError, match="not a fused optimizer"):
        M.FusedMultiOptimizer({"A": torch.optim.AdamW(w())}, nonfinite_guard=True)
    M.FusedMultiOptimizer({"A": torch.optim.AdamW(w())})  # neither clip nor guard: still accepted
    with pytest.raises(ValueError, match="own nonfinite_guard"):
        M.FusedMultiOptimizer({"A": M.FusedAdamW(w(), nonfinite_guard=True)}, nonfinite_guard=True)
    guarded = M.FusedAdamW(w(), nonfinite_guard=True)
    with pytest.raises(ValueError, match="nonfinite_guard is set"):
        guarded.use_shared_clip(torch.zeros(1), 1.0, guard=L.StepGuard())
    plain = M.FusedAdamW(w())
    plain.use_shared_clip(torch.zeros(1), None, guard=L.StepGuard())  # a guarded run without a clip
    with pytest.raises(ValueError, match="max_norm"):
        plain.use_shared_clip(torch.zeros(1), None)


def test_build_optimizer_passes_the_guard_through():
    from linnaeus_amd.config import ConfigNode
    from linnaeus_amd.optim import build_optimizer

    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4))
    for name, kind in [("adamw", "FusedAdamW"), ("sgd", "FusedSGD"), ("ademamix", "FusedAdEMAMix"), ("muon", "FusedMultiOptimizer")]:
        cfg = ConfigNode({"OPTIMIZER": {"NAME": name}, "LR_SCHEDULER": {"BASE_LR": 1e-3}, "TRAIN": {"CLIP_GRAD": 1.0}})
        on, off = build_optimizer(cfg, model, nonfinite_guard=True), build_optimizer(cfg, model)
        assert type(on).__name__ == kind and on.nonfinite_guard and on._step_supports_amp_scaling and not off.nonfinite_guard
        if name == "muon":  # one pass decides for all: the sub-optimizers carry no guard of their own
            assert not any(o.nonfinite_guard for o in on.optimizers.values())


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_guard_mirrors_have_the_sizes_the_c_compiler_gives(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in L.GUARD_STRUCTS) +
                   '    printf("guard_offset %zu\\n", offsetof(lnx_muon_step_args, guard));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in L.GUARD_STRUCTS.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    assert int(got["guard_offset"]) == L.MuonStepArgs.guard.offset
    assert [f[0] for f in L.StepGuard._fields_] == ["found_inf", "grad_scale", "flag", "skipped"]
    assert L.lib().lnx_version() >= 117


def test_guarded_entry_points_validate_on_the_host():
    """a NULL table or a guard without its flag is refused with a message and before any launch (the pointers are never dereferenced)"""
    lib = L.lib()
    fake = 0x1000
    ok, no_flag, no_count = L.StepGuard(), L.StepGuard(), L.StepGuard()
    ok.flag, ok.skipped = fake, fake
    no_flag.skipped = fake
    no_count.flag = fake
    before = lib.lnx_optim_launches()
    # the norm pass: needs the flag and the counter
    assert lib.lnx_grad_sumsq_guarded(None, 1, 1, fake, fake, C.byref(ok), None) != 0
    assert b"lnx_grad_sumsq" in lib.lnx_last_error()
    for bad in (no_flag, no_count):
        assert lib.lnx_grad_sumsq_guarded(fake, 1, 1, fake, fake, C.byref(bad), None) != 0
        assert b"lnx_grad_sumsq_guarded" in lib.lnx_last_error() and b"flag" in lib.lnx_last_error()
    # the three steps: need the flag
    ha, he, hs = L.AdamWHyper(), L.AdEMAMixHyper(), L.SGDHyper()
    for h in (ha, he):
        h.ngroups = 1
        h.bias_c1[0], h.bias_c2[0] = 0.1, 0.001
    hs.ngroups = 1
    calls = {
        "lnx_adamw_step": lambda table, g: lib.lnx_adamw_step_guarded(table, 1, 1, C.byref(ha), None, 0.0, C.byref(g), None),
        "lnx_ademamix_step": lambda table, g: lib.lnx_ademamix_step_guarded(table, fake, 1, 1, C.byref(he), None, 0.0, C.byref(g), None),
        "lnx_sgd_step": lambda table, g: lib.lnx_sgd_step_guarded(table, 1, 1, C.byref(hs), None, 0.0, C.byref(g), None),
    }
    for name, call in calls.items():
        assert call(None, ok) != 0
        assert name.encode() in lib.lnx_last_error(), lib.lnx_last_error()
        assert call(fake, no_flag) != 0
        assert (name + "_guarded").encode() in lib.lnx_last_error() and b"no flag" in lib.lnx_last_error(), lib.lnx_last_error()
    # Muon: the guard rides in the argument struct
    from linnaeus_amd.optim import muon_layout

    mats, tiles, info = muon_layout([(8, 8)])
    mats[0].p = mats[0].g = mats[0].buf = fake
    a = L.MuonStepArgs()
    a.n, a.mats, a.mats_dev, a.tiles_dev = 1, C.addressof(mats), fake, fake
    a.workspace, a.workspace_bytes, a.partials = 0x10000, info.workspace_bytes, fake
    a.guard = C.pointer(no_flag)
    m0 = lib.lnx_muon_launches()
    assert lib.lnx_muon_step(C.byref(a), None) != 0
    assert b"lnx_muon_step" in lib.lnx_last_error() and b"no flag" in lib.lnx_last_error()
    assert lib.lnx_optim_launches() == before and lib.lnx_muon_launches() == m0  # nothing was launched
