"""The non-finite guard of the fused optimizers on the GPU (`nonfinite_guard=True`, csrc/optim.hip and csrc/muon.hip).

Inputs.  Elementwise optimizers: tensors of 1, 3, 5, 1023, 4096, 4097, 37 and 8199 elements -- the scalar tail, exactly one workgroup
(4096 elements), a workgroup seam and a three-workgroup tensor -- the 37-element one with a `.grad` that starts one float into a buffer
(the path without 16-byte accesses).  Muon: five of the matrices of tests/test_gpu_muon_fused.py (wide, padded in both directions, a
flattened 4-D weight, odd square, 5 tiles x 9 K steps).  Gradients are +-2^k, k in [-10, 10]: no square is subnormal, no square
scaled by 2^32 overflows, and sum of squares and norm at scale 2^16 are exactly 2^32 and 2^16 times the unscaled ones, so a scaled run
can be compared with the unscaled one bit for bit.

Bounds.  Where a run with a skipped step must EQUAL another run (Muon; SGD wherever no buffer is created on the skipped step, and at
dampening 0 there too; guard on against guard off on clean gradients; scale 2^16 against no scale) the comparison is torch.equal.
AdamW and AdEMAMix count attempted steps, so after a skip they are compared with tests/optim_guard_ref.py within the bounds of
tests/test_gpu_optim_build.py: parameters rtol 2e-6 / atol 2e-7, states the same rtol and atol 8 ulps of the largest term that
entered them (|g|, g^2).  The one SGD run that is compared with the restatement (dampening 0.1, buffer created on the skipped step) takes
steps of lr |buffer| up to about 25 with these gradients, so its parameters pass through values far above where they end: their atol
is 8 ulps of the largest |p| or lr |buffer| the restatement sees, the same form, and never less than 2e-7."""
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd.config import ConfigNode
from tests.optim_guard_ref import GuardRef, run as ref_run

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-6, 2e-7
ULP8 = 8 * 2.0 ** -23
SIZES = [1, 3, 5, 1023, 4096, 4097, 37, 8199]
OFFSET = 37  # the tensor whose gradient is not 16-byte aligned
MUON_SHAPES = [(48, 192), (40, 100), (16, 1, 7, 7), (33, 33), (136, 264)]
GROUPS = {
    "adamw": dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05),
    "ademamix": dict(lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0.05, alpha=5.0, T_alpha_beta3=10),
    "sgd": dict(lr=0.01, momentum=0.9, dampening=0.0, nesterov=True, weight_decay=0.05),
    "sgd_damp": dict(lr=0.01, momentum=0.9, dampening=0.1, nesterov=False, weight_decay=0.05),
    "muon": dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5),
}
KINDS = ["adamw", "ademamix", "sgd", "muon", "multi"]  # multi: FusedMultiOptimizer of Muon + AdamW
POISONS = {"inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "3e19": 3e19}  # 3e19 is finite; its square is not
BIG_CLIP = 1e6  # above any norm these gradients can have (at most sqrt(68 k elements) 2^10 = 2.7e5): the clip coefficient is exactly 1


def optim():
    from linnaeus_amd import optim as M

    return M


def shapes_of(kind):
    flat = [(n,) for n in SIZES]
    return MUON_SHAPES if kind == "muon" else flat + MUON_SHAPES if kind == "multi" else flat


def pow2(shape, gen):
    """+-2^k, k uniform in [-10, 10]"""
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2 - 1
    g = torch.ldexp(sign, torch.randint(-10, 11, shape, generator=gen))
    assert (torch.frexp(g.abs()).mantissa == 0.5).all() and g.abs().max() <= 1024 and g.abs().min() >= 2.0 ** -10
    return g


def inputs(kind, steps, seed=41):
    gen = torch.Generator().manual_seed(seed)
    shapes = shapes_of(kind)
    return [torch.randn(*s, generator=gen) * 0.1 for s in shapes], [[pow2(s, gen) for s in shapes] for _ in range(steps)]


def build(kind, values, guard, clip):
    M = optim()
    params = [torch.nn.Parameter(v.cuda()) for v in values]
    kw = dict(max_grad_norm=clip, nonfinite_guard=guard)
    if kind == "multi":
        n = len(SIZES)  # the union table lists ADAMW's tensors first (sorted names)
        return M.FusedMultiOptimizer({"MUON": M.FusedMuon(params[n:], **GROUPS["muon"]), "ADAMW": M.FusedAdamW(params[:n], **GROUPS["adamw"])}, **kw), params
    cls = {"adamw": M.FusedAdamW, "ademamix": M.FusedAdEMAMix, "sgd": M.FusedSGD, "muon": M.FusedMuon}[kind.split("_")[0]]
    return cls(params, **GROUPS[kind], **kw), params


def set_grads(params, grads, scale=1.0):
    for p, g in zip(params, grads):
        g = g * scale
        if tuple(g.shape) == (OFFSET,):
            flat = torch.zeros(OFFSET + 1, device="cuda")
            flat[1:] = g.cuda()
            p.grad = flat[1:]
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = g.cuda()


def subs(opt):
    return [opt.optimizers[k] for k in sorted(opt.optimizers)] if hasattr(opt, "optimizers") else [opt]


def state_tensors(opt, params):
    """every parameter and every state tensor, in a fixed order"""
    out = []
    for o in subs(opt):
        for p in (q for g in o.param_groups for q in g["params"]):
            out.append(p.detach())
            out += [v for _, v in sorted(o.state.get(p, {}).items()) if isinstance(v, torch.Tensor)]
    assert len(out) > len(params)
    return out


def snapshot(opt, params):
    """a copy of everything a step could write: parameters, state tensors, gradients, Muon's whole workspace"""
    out = [t.clone() for t in state_tensors(opt, params)] + [p.grad.clone() for p in params]
    return out + [o._dev[2].clone() for o in subs(opt) if getattr(o, "_dev", None) is not None]


def same_bits(a, b):
    """torch.equal on the bytes (NaN == NaN)"""
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)) for x, y in zip(a, b))


def poison_at(shapes, where):
    """(tensor, flat index): the first element of the first tensor, the last element of the last tensor (in its scalar tail) or an
    element in a middle workgroup of the last tensor"""
    n = 1
    for d in shapes[-1]:
        n *= d
    assert n > 2 * 4096
    return {"first": (0, 0), "last": (len(shapes) - 1, n - 1), "middle": (len(shapes) - 1, (n // 4096 // 2) * 4096 + 100)}[where]


def muon_padding_is_zero(opt):
    from tests.test_gpu_muon_fused import padding_is_zero

    return all(padding_is_zero(o) for o in subs(opt) if getattr(o, "_dev", None) is not None)


def check_against_restatement(kind, opt, params, values, seq, poisoned, label):
    """the elementwise tensors of `params` (all of them, or the AdamW part of the multi-optimizer) against tests/optim_guard_ref.py"""
    ref_kind = "adamw" if kind == "multi" else kind
    n = len(SIZES)
    dtype = torch.float64 if ref_kind == "ademamix" else torch.float32
    ref = GuardRef(ref_kind.split("_")[0], [torch.nn.Parameter(v.to(dtype).clone()) for v in values[:n]], GROUPS[ref_kind])
    big = [0.0] * n  # SGD only: the largest |p| and lr |buffer| of the run (see the module docstring)
    for s, grads in enumerate(seq):
        ref_params = ref_run(ref, [grads[:n]], (0,) if s in poisoned else ())
        if ref_kind.startswith("sgd"):
            for i, q in enumerate(ref_params):
                buf = ref.state_of(q).get("momentum_buffer")
                big[i] = max(big[i], float(q.detach().abs().max()), 0.0 if buf is None else GROUPS[ref_kind]["lr"] * float(buf.abs().max()))
    sub = opt.optimizers["ADAMW"] if kind == "multi" else opt
    for i, (p, q) in enumerate(zip(params[:n], ref_params)):
        torch.testing.assert_close(p.detach().cpu().double(), q.detach().double(), rtol=RTOL, atol=max(ATOL, ULP8 * big[i]),
                                   msg=lambda m: f"{label} size {SIZES[i]}: {m}")
        gmax = max(float(g[i].abs().max()) for s, g in enumerate(seq) if s not in poisoned)
        st, want = sub.state[p], ref.state_of(q)
        for k, w in want.items():
            if k == "step":
                assert int(st["step"]) == int(w) == len(seq)  # attempted steps
            else:
                atol = ULP8 * (gmax * gmax if k == "exp_avg_sq" else gmax)
                torch.testing.assert_close(st[k].cpu().double(), w.double(), rtol=RTOL, atol=atol, msg=lambda m: f"{label} size {SIZES[i]} {k}: {m}")


# ------------------------------------------------------------------------------------------------------------------ skip
SKIP_CASES = [(p, w, BIG_CLIP) for p in POISONS for w in ("first", "last", "middle")] + [("inf", w, None) for w in ("first", "last", "middle")]


@pytest.mark.parametrize("poison,where,clip", SKIP_CASES, ids=[f"{p}-{w}-{'clip' if c else 'noclip'}" for p, w, c in SKIP_CASES])
@pytest.mark.parametrize("kind", KINDS)
def test_a_poisoned_step_writes_nothing_and_the_run_goes_on(kind, poison, where, clip):
    values, seq = inputs(kind, 5)
    t, i = poison_at(shapes_of(kind), where)
    seq[1][t].view(-1)[i] = POISONS[poison]
    opt, params = build(kind, values, True, clip)
    twin, twin_params = build(kind, values, False, clip)  # never sees the poisoned step
    for s, grads in enumerate(seq):
        set_grads(params, grads)
        if s != 1:
            opt.step()
            assert not bool(opt.last_step_skipped())
            set_grads(twin_params, grads)
            twin.step()
            continue
        before = snapshot(opt, params)
        opt.step()
        assert same_bits(snapshot(opt, params), before)
        assert int(opt.skipped_steps()) == 1 and bool(opt.last_step_skipped())
        assert not torch.isfinite(opt.grad_norm())
    assert int(opt.skipped_steps()) == 1 and muon_padding_is_zero(opt)
    assert all(torch.isfinite(x).all() for x in state_tensors(opt, params))
    if kind in ("muon", "sgd"):
        assert same_bits(state_tensors(opt, params), state_tensors(twin, twin_params))
    else:
        check_against_restatement(kind, opt, params, values, seq, (1,), f"{kind} {poison} {where}")
    if kind == "multi":
        n = len(SIZES)
        assert same_bits(state_tensors(opt.optimizers["MUON"], params[n:]), state_tensors(twin.optimizers["MUON"], twin_params[n:]))


@pytest.mark.parametrize("kind", KINDS + ["sgd_damp"])
def test_a_poisoned_first_step_creates_zero_state(kind):
    """the state is created on the host during the skipped step: moments and momentum buffers must read as zero afterwards (FusedSGD's
    buffer is otherwise uninitialised memory that the kernel fills), and Muon's workspace stays zero"""
    values, seq = inputs(kind, 4)
    seq[0][0].view(-1)[0] = float("inf")
    opt, params = build(kind, values, True, BIG_CLIP)
    twin, twin_params = build(kind, values, False, BIG_CLIP)
    set_grads(params, seq[0])
    before = [p.detach().clone() for p in params] + [p.grad.clone() for p in params]
    opt.step()
    assert same_bits([p.detach() for p in params] + [p.grad for p in params], before)
    assert int(opt.skipped_steps()) == 1 and bool(opt.last_step_skipped())
    for o in subs(opt):
        for p, st in o.state.items():
            assert all(not v.any() for v in st.values() if isinstance(v, torch.Tensor))
        if getattr(o, "_dev", None) is not None:
            assert not o._dev[2].any()
    for grads in seq[1:]:
        set_grads(params, grads)
        opt.step()
        set_grads(twin_params, grads)
        twin.step()
    assert int(opt.skipped_steps()) == 1 and not bool(opt.last_step_skipped()) and muon_padding_is_zero(opt)
    if kind in ("muon", "sgd"):  # no step-dependent term; at dampening 0 the zero buffer gives momentum 0 + g = g, torch's clone
        assert same_bits(state_tensors(opt, params), state_tensors(twin, twin_params))
    else:  # sgd_damp: (1 - dampening) g where torch clones g, the stated difference, as the restatement has it
        check_against_restatement(kind, opt, params, values, seq, (0,), kind)
    if kind == "multi":
        n = len(SIZES)
        assert same_bits(state_tensors(opt.optimizers["MUON"], params[n:]), state_tensors(twin.optimizers["MUON"], twin_params[n:]))
    if kind == "sgd_damp":
        assert not same_bits(state_tensors(opt, params), state_tensors(twin, twin_params))


@pytest.mark.parametrize("kind", KINDS)
def test_found_inf_alone_skips_the_step(kind):
    """GradScaler's verdict feeds the flag even when the sum of squares is finite (a non-finite gradient of ANOTHER optimizer)"""
    values, seq = inputs(kind, 3)
    opt, params = build(kind, values, True, None)
    set_grads(params, seq[0])
    opt.step()
    set_grads(params, seq[1])
    before = snapshot(opt, params)
    opt.found_inf = torch.ones((), device="cuda")
    opt.step()
    del opt.found_inf
    assert same_bits(snapshot(opt, params), before)
    assert int(opt.skipped_steps()) == 1 and bool(opt.last_step_skipped()) and torch.isfinite(opt.grad_norm())
    opt.found_inf = torch.zeros((), device="cuda")
    opt.step()
    assert int(opt.skipped_steps()) == 1 and not bool(opt.last_step_skipped())
    assert not same_bits(snapshot(opt, params), before)


# ------------------------------------------------------------------------------------------------------------------ clean gradients
@pytest.mark.parametrize("clip", [None, 1.0, BIG_CLIP], ids=["noclip", "clip1", "clip1e6"])
@pytest.mark.parametrize("kind", KINDS)
def test_the_guard_changes_nothing_on_finite_gradients(kind, clip):
    values, seq = inputs(kind, 3)
    on, on_params = build(kind, values, True, clip)
    off, off_params = build(kind, values, False, clip)
    for grads in seq:
        set_grads(on_params, grads)
        set_grads(off_params, grads)
        on.step()
        off.step()
        want = sum(float(g.double().pow(2).sum()) for g in grads) ** 0.5
        torch.testing.assert_close(float(on.grad_norm()), want, rtol=1e-5, atol=0.0)  # also without a clip
        if clip is not None:
            torch.testing.assert_close(on.grad_norm(), off.grad_norm(), rtol=1e-6, atol=0.0)
        else:
            assert off.grad_norm() is None
        assert not bool(on.last_step_skipped())
    assert int(on.skipped_steps()) == 0
    assert off.skipped_steps() is None and off.last_step_skipped() is None
    assert same_bits(state_tensors(on, on_params), state_tensors(off, off_params))


# ------------------------------------------------------------------------------------------------------------------ scale
@pytest.mark.parametrize("clip", [None, 1.0], ids=["noclip", "clip1"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_power_of_two_grad_scale_gives_the_unscaled_bits(kind, clip):
    values, seq = inputs(kind, 3)
    plain, plain_params = build(kind, values, True, clip)
    scaled, scaled_params = build(kind, values, True, clip)
    for grads in seq:
        set_grads(plain_params, grads)
        set_grads(scaled_params, grads, scale=2.0 ** 16)
        plain.step()
        scaled.grad_scale, scaled.found_inf = torch.tensor(2.0 ** 16, device="cuda"), torch.zeros((), device="cuda")  # as GradScaler.step sets them
        scaled.step()
        del scaled.grad_scale, scaled.found_inf
        assert torch.equal(plain.grad_norm(), scaled.grad_norm()) and torch.isfinite(plain.grad_norm())
    assert int(scaled.skipped_steps()) == 0
    assert same_bits(state_tensors(plain, plain_params), state_tensors(scaled, scaled_params))
    if clip is not None:  # the clip did bite: not the unclipped run
        free, free_params = build(kind, values, True, None)
        set_grads(free_params, seq[0])
        free.step()
        assert float(free.grad_norm()) > 100 * clip


# ------------------------------------------------------------------------------------------------------------------ GradScaler
POISONED = 2


@pytest.mark.parametrize("flow", [1, 2], ids=["scale-step-update", "scale-unscale-step-update"])
@pytest.mark.parametrize("kind", ["adamw", "sgd", "muon+adamw"])
def test_gradscaler_end_to_end_without_host_synchronisation(kind, flow):
    """torch.amp.GradScaler("cuda") around the guarded optimizer on a tiny Linear stack, one iteration poisoned, everything after the
    first (table-building) iteration under torch.cuda.set_sync_debug_mode("error").  The gradients each step saw are copied to pinned
    memory without a sync and replayed through the restatement afterwards."""
    M = optim()
    torch.manual_seed(5)
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4)).cuda()
    params = list(model.parameters())
    init = [p.detach().cpu().clone() for p in params]
    if kind == "muon+adamw":
        cfg = ConfigNode({"OPTIMIZER": {"NAME": "muon"}, "LR_SCHEDULER": {"BASE_LR": 1e-3}, "TRAIN": {"CLIP_GRAD": BIG_CLIP}})
        opt = M.build_optimizer(cfg, model, nonfinite_guard=True)
        assert type(opt).__name__ == "FusedMultiOptimizer" and sorted(opt.optimizers) == ["ADAMW", "MUON"]
    else:
        opt = {"adamw": M.FusedAdamW, "sgd": M.FusedSGD}[kind](params, **GROUPS[kind], max_grad_norm=BIG_CLIP, nonfinite_guard=True)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    steps = 5
    xs, ys = torch.randn(steps, 32, 8, device="cuda"), torch.randn(steps, 32, 4, device="cuda")
    seen = [[torch.empty(p.shape).pin_memory() for p in params] for _ in range(steps)]
    unchanged, changed = [], []
    for p in params:
        p.grad = torch.zeros_like(p)  # the same gradient tensors at every step: the tables are built once

    def iteration(s):
        opt.zero_grad(set_to_none=False)
        scaler.scale(torch.nn.functional.mse_loss(model(xs[s]), ys[s])).backward()
        if s == POISONED:
            params[0].grad[0, :1].fill_(float("inf"))  # (an indexed assignment of a Python number copies it from the host: a sync)
        if flow == 2:
            scaler.unscale_(opt)
        for dst, p in zip(seen[s], params):
            dst.copy_(p.grad, non_blocking=True)
        before = [p.detach().clone() for p in params]
        scaler.step(opt)
        scaler.update()
        same = torch.stack([(p.detach() == b).all() for p, b in zip(params, before)])
        (unchanged if s == POISONED else changed).append(same)

    iteration(0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(1, steps):
            iteration(s)
        skipped, last, norm = opt.skipped_steps(), opt.last_step_skipped(), opt.grad_norm()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(skipped) == 1 and not bool(last) and torch.isfinite(norm)
    assert scaler.get_scale() == 2.0 ** 15  # halved once, after the poisoned step
    assert unchanged[0].all() and not any(c.any() for c in changed)
    assert all(torch.isfinite(p).all() for p in params)
    if kind == "muon+adamw":
        return
    scale_at = lambda s: 1.0 if flow == 2 else 2.0 ** (16 if s <= POISONED else 15)  # noqa: E731  (unscale_ has divided it out already)
    seq = [[g / scale_at(s) for g in seen[s]] for s in range(steps)]
    ref = GuardRef(kind, [torch.nn.Parameter(v.clone()) for v in init], GROUPS[kind])
    for p, q in zip(params, ref_run(ref, seq, (POISONED,))):
        torch.testing.assert_close(p.detach().cpu(), q.detach(), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------------------------------------------ launches
@pytest.mark.parametrize("kind", KINDS)
def test_launch_counts(kind):
    """guard on with a clip: exactly the clipped step's launches (the fold launch decides); guard on without a clip: the unclipped
    step's plus the two of the norm pass; guard off: as before"""
    lib = L.lib()
    ns = GROUPS["muon"]["ns_steps"]
    update = 0 if kind == "muon" else 1  # launches counted by lnx_optim_launches besides the norm pass
    muon = 0 if kind not in ("muon", "multi") else 3 * ns + 3
    values, seq = inputs(kind, 1)
    for guard, clip, norm_pass in [(False, None, 0), (False, 1.0, 2), (True, 1.0, 2), (True, None, 2)]:
        opt, params = build(kind, values, guard, clip)
        set_grads(params, seq[0])
        opt.step()
        torch.cuda.synchronize()
        o0, m0 = lib.lnx_optim_launches(), lib.lnx_muon_launches()
        opt.step()
        opt.step()
        torch.cuda.synchronize()
        assert lib.lnx_optim_launches() - o0 == 2 * (update + norm_pass), (guard, clip)
        assert lib.lnx_muon_launches() - m0 == 2 * muon, (guard, clip)
