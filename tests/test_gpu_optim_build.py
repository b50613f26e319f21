"""The configured optimizer on the GPU: FusedSGD against an fp64 restatement and against torch.optim.SGD, the shared global clip of
FusedMultiOptimizer on an exactly representable probe, lnx_muon_step's clip tail driven directly, the union norm, the replay of the
reference's three recorded steps (tests/golden/optim_step.npz, written by tests/golden/gen/make_golden_optim_build.py), launch counts
without host synchronisation, and build_optimizer end to end on the tiny model.

Tolerances.  Parameters: rtol 2e-6 / atol 2e-7, the bound tests/test_optim.py uses for FusedAdamW against torch (on the CPU,
torch.optim.SGD in fp32 against the fp64 restatement below stays within about a tenth of it for inputs of this kind).  Momentum buffers and EMA
states: the same rtol, atol 8 ulps (2^-20) of the largest term that entered them (|coef g| + wd |p| for SGD, |g| and g^2 for AdamW), the
form of tests/test_ademamix.py: they are sums of terms that can cancel."""
import ctypes as C

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd.config import ConfigNode
from tests import muon_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-6, 2e-7
ULP8 = 8 * 2.0 ** -23
# every vector-round (1024), tail and workgroup (4096) seam
SIZES = [1, 3, 4, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
SGD_GROUPS = [dict(lr=0.01, momentum=0.9, dampening=0.0, weight_decay=0.05, nesterov=True),
              dict(lr=0.02, momentum=0.0, dampening=0.0, weight_decay=0.01, nesterov=False),
              dict(lr=0.015, momentum=0.8, dampening=0.1, weight_decay=0.0, nesterov=False)]
LATE = (0, SIZES.index(1025))  # (group, tensor): no gradient at the first step, so it takes the first-step slot at the second
MUON_G = dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5)
ADAMW_G = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
ADEMAMIX_G = dict(lr=1e-3, betas=(0.9, 0.999, 0.9999), eps=1e-8, weight_decay=0.05, alpha=5.0, T_alpha_beta3=10)
SGD_G = dict(lr=0.01, momentum=0.9, nesterov=True, weight_decay=0.05)


def optim():
    from linnaeus_amd import optim as M

    return M


def device_params(values, offset=False):
    """one Parameter per CPU tensor; with offset, views one element into a larger buffer (4 bytes off a 16-byte boundary)"""
    out = []
    for v in values:
        if offset:
            flat = torch.zeros(v.numel() + 1, device="cuda")
            flat[1:] = v.flatten().cuda()
            out.append(torch.nn.Parameter(flat[1:].view(v.shape)))
            assert out[-1].data_ptr() % 16 == 4
        else:
            out.append(torch.nn.Parameter(v.cuda()))
    return out


def set_grad(p, g, offset=False):
    if g is None:
        p.grad = None
    elif offset:
        flat = torch.zeros(g.numel() + 1, device="cuda")
        flat[1:] = g.flatten().cuda()
        p.grad = flat[1:].view(g.shape)
    else:
        p.grad = g.cuda()


# ------------------------------------------------------------------------------------------------------------------ SGD
def sgd_ref_step(p, g, buf, group, coef):
    """the rule of lnx_sgd_step in fp64; returns the new buffer (None without momentum); p is updated in place"""
    g = g * coef + group["weight_decay"] * p
    if group["momentum"] != 0:
        buf = g.clone() if buf is None else group["momentum"] * buf + (1 - group["dampening"]) * g
        g = g + group["momentum"] * buf if group["nesterov"] else buf
    p -= group["lr"] * g
    return buf


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "offset"])
@pytest.mark.parametrize("clip", [None, 0.5, 1e6])
def test_sgd_against_fp64(clip, offset):
    gen = torch.Generator().manual_seed(31)
    init = [[torch.randn(n, generator=gen) * 0.1 for n in SIZES] for _ in SGD_GROUPS]
    params = [device_params(v, offset) for v in init]
    opt = optim().FusedSGD([dict(params=ps, **g) for ps, g in zip(params, SGD_GROUPS)], lr=0.1, max_grad_norm=clip)
    ref_p = [[v.double().clone() for v in grp] for grp in init]
    ref_buf = [[None] * len(SIZES) for _ in SGD_GROUPS]
    big = [[0.0] * len(SIZES) for _ in SGD_GROUPS]
    for s in range(4):
        grads = [[None if (s == 0 and (gi, i) == LATE) else torch.randn(n, generator=gen) for i, n in enumerate(SIZES)] for gi in range(len(SGD_GROUPS))]
        for gi, grp in enumerate(params):
            for i, p in enumerate(grp):
                set_grad(p, grads[gi][i], offset)
        total = sum(float(g.double().pow(2).sum()) for grp in grads for g in grp if g is not None) ** 0.5
        coef = 1.0 if clip is None else min(1.0, clip / (total + 1e-6))
        opt.step()
        if clip is not None:
            np.testing.assert_allclose(float(opt.grad_norm()), total, rtol=1e-5, atol=1e-6)
        for gi, group in enumerate(SGD_GROUPS):
            for i, p in enumerate(params[gi]):
                g = grads[gi][i]
                if g is not None:
                    big[gi][i] = max(big[gi][i], float((g.double().abs() * coef + group["weight_decay"] * ref_p[gi][i].abs()).max()))
                    ref_buf[gi][i] = sgd_ref_step(ref_p[gi][i], g.double(), ref_buf[gi][i], group, coef)
                    assert torch.equal(p.grad.cpu(), g)  # the gradient is read, never written
                torch.testing.assert_close(p.detach().cpu().double(), ref_p[gi][i], rtol=RTOL, atol=ATOL, msg=lambda m: f"group {gi} size {SIZES[i]} step {s + 1}: {m}")
                st = opt.state.get(p, {})
                if ref_buf[gi][i] is None:
                    assert "momentum_buffer" not in st  # momentum 0, or no gradient yet
                else:
                    torch.testing.assert_close(st["momentum_buffer"].cpu().double(), ref_buf[gi][i], rtol=RTOL, atol=ULP8 * big[gi][i],
                                               msg=lambda m: f"buffer, group {gi} size {SIZES[i]} step {s + 1}: {m}")


def test_sgd_against_torch_and_state_dict_exchange():
    gen = torch.Generator().manual_seed(32)
    init = [torch.randn(n, generator=gen) * 0.1 for n in SIZES]
    mine, theirs = device_params(init), device_params(init)
    o = optim().FusedSGD(mine, **SGD_G)
    t = torch.optim.SGD(theirs, **SGD_G)
    big = 0.0
    for s in range(4):
        for a, b, n in zip(mine, theirs, SIZES):
            g = torch.randn(n, generator=gen)
            big = max(big, float(g.abs().max()) + SGD_G["weight_decay"] * float(a.detach().abs().max()))
            set_grad(a, g)
            set_grad(b, g)
        o.step()
        t.step()
        for a, b, n in zip(mine, theirs, SIZES):
            torch.testing.assert_close(a.detach(), b.detach(), rtol=RTOL, atol=ATOL, msg=lambda m: f"size {n} step {s + 1}: {m}")
        if s == 1:  # the two swap their states and go on
            sd_o, sd_t = o.state_dict(), t.state_dict()
            assert set(sd_o["state"][0]) == set(sd_t["state"][0]) == {"momentum_buffer"}
            o.load_state_dict(sd_t)
            t.load_state_dict(sd_o)
    for a, b in zip(mine, theirs):
        torch.testing.assert_close(o.state[a]["momentum_buffer"], t.state[b]["momentum_buffer"], rtol=RTOL, atol=ULP8 * big)


# ------------------------------------------------------------------------------------------------------------------ the exact probe
PROBE = {"MUON": [(48, 192), (40, 100), (16, 1, 7, 7)], "ADAMW": [(4097,), (33, 7)], "ADEMAMIX": [(1025,), (64, 3), (41890,)], "SGD": [(4096,), (5,)]}


def make_sub(name, params):
    M = optim()
    kind = name.split("_")[0]
    return {"MUON": lambda: M.FusedMuon(params, **MUON_G), "ADAMW": lambda: M.FusedAdamW(params, **ADAMW_G),
            "ADEMAMIX": lambda: M.FusedAdEMAMix(params, **ADEMAMIX_G), "SGD": lambda: M.FusedSGD(params, **SGD_G)}[kind]()


def states_equal(a_opt, a_params, b_opt, b_params):
    for p, q in zip(a_params, b_params):
        if not torch.equal(p.detach(), q.detach()):
            return False
        sa, sb = a_opt.state[p], b_opt.state[q]
        if set(sa) != set(sb):
            return False
        for k in sa:
            if not torch.equal(torch.as_tensor(sa[k]).cpu(), torch.as_tensor(sb[k]).cpu()):
                return False
    return True


def test_exact_clip_probe():
    """2^16 gradient elements of +-0.5: the sum of squares is 2^14 in any order, the norm 128, 128 + 1e-6 rounds to 128, so a clip at 32
    scales by exactly 0.25 -- and every sub-optimizer must then be bit-identical to itself stepping alone, unclipped, on +-0.125."""
    assert sum(int(np.prod(s)) for v in PROBE.values() for s in v) == 2 ** 16
    gen = torch.Generator().manual_seed(33)
    init = {k: [torch.randn(*s, generator=gen) * 0.1 for s in v] for k, v in PROBE.items()}
    together = {k: device_params(v) for k, v in init.items()}
    alone = {k: device_params(v) for k, v in init.items()}
    multi = optim().FusedMultiOptimizer({k: make_sub(k, ps) for k, ps in together.items()}, max_grad_norm=32.0)
    solo = {k: make_sub(k, ps) for k, ps in alone.items()}
    for s in range(2):
        given = {}
        for k, shapes in PROBE.items():
            for i, shape in enumerate(shapes):
                g = (torch.randint(0, 2, shape, generator=gen).float() - 0.5)
                given[k, i] = g
                set_grad(together[k][i], g)
                set_grad(alone[k][i], g * 0.25)
        multi.step()
        for o in solo.values():
            o.step()
        pre, post, returned = multi.grad_norms()
        assert torch.equal(pre, torch.tensor(128.0, device="cuda")) and torch.equal(post, torch.tensor(32.0, device="cuda")) and torch.equal(returned, pre)
        assert torch.equal(multi.grad_norm(), pre)
        for k in PROBE:
            assert states_equal(multi.optimizers[k], together[k], solo[k], alone[k]), (k, s)
            for i, p in enumerate(together[k]):
                assert torch.equal(p.grad.cpu(), given[k, i])  # clip_grad_norm_ scales .grad; here it stays as given


# ------------------------------------------------------------------------------------------------------------------ raw Muon entry
def raw_muon_step(values, grads, group, sumsq=None, max_norm=0.0):
    """lnx_muon_step through ctypes on fresh buffers; returns (parameters, momentum buffers) on the CPU"""
    ps, gs = [v.cuda() for v in values], [g.cuda() for g in grads]
    bufs = [torch.zeros_like(p) for p in ps]
    shapes = [(p.size(0), p.numel() // p.size(0)) for p in ps]
    mats, tiles, info = optim().muon_layout(shapes)
    for m, p, g, b, (rows, cols) in zip(mats, ps, gs, bufs, shapes):
        m.p, m.g, m.buf = p.data_ptr(), g.data_ptr(), b.data_ptr()
        m.ns_steps, m.nesterov = group["ns_steps"], 1 if group["nesterov"] else 0
        m.momentum, m.omm = group["momentum"], 1 - group["momentum"]
        m.decay, m.step = 1 - group["lr"] * group["weight_decay"], group["lr"] * max(1, rows / cols) ** 0.5
    table = torch.frombuffer(bytearray(bytes(mats)), dtype=torch.uint8).cuda()
    tiles_d = torch.from_numpy(tiles).cuda()
    ws = torch.zeros(info.workspace_bytes, device="cuda", dtype=torch.uint8)
    part = torch.empty(info.total_blocks, device="cuda", dtype=torch.float32)
    a = L.MuonStepArgs()
    a.n, a.mats, a.mats_dev, a.tiles_dev = len(ps), C.addressof(mats), table.data_ptr(), tiles_d.data_ptr()
    a.workspace, a.workspace_bytes, a.partials = ws.data_ptr(), ws.numel(), part.data_ptr()
    if sumsq is not None:
        a.sumsq = sumsq.data_ptr()
    a.max_norm = max_norm
    L.check(L.lib().lnx_muon_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_muon_step")
    torch.cuda.synchronize()
    for g, g0 in zip(gs, grads):
        assert torch.equal(g.cpu(), g0)
    return [p.cpu() for p in ps], [b.cpu() for b in bufs]


def test_muon_entry_point_clips_by_a_written_sum_of_squares():
    gen = torch.Generator().manual_seed(34)
    shapes = [(48, 192), (40, 100), (16, 1, 7, 7)]
    values = [torch.randn(*s, generator=gen) * 0.1 for s in shapes]
    grads = [torch.randn(*s, generator=gen) for s in shapes]
    quarter = [g * 0.25 for g in grads]
    sumsq = torch.tensor([2.0 ** 40], device="cuda")  # norm 2^20 (+ 1e-6 rounds away); max_norm 2^18: coef 0.25 exactly
    clipped = raw_muon_step(values, grads, MUON_G, sumsq, 2.0 ** 18)
    scaled = raw_muon_step(values, quarter, MUON_G)  # sumsq NULL
    for a, b in zip(clipped[0] + clipped[1], scaled[0] + scaled[1]):
        assert torch.equal(a, b)
    # sumsq NULL, max_norm <= 0 with a pointer, and a norm under the clip: the step as it always was
    ps = device_params(values)
    for p, g in zip(ps, quarter):
        set_grad(p, g)
    opt = optim().FusedMuon(ps, **MUON_G)
    opt.step()
    torch.cuda.synchronize()
    today = [p.detach().cpu() for p in ps], [opt.state[p]["momentum_buffer"].cpu() for p in ps]
    for other in (scaled, raw_muon_step(values, quarter, MUON_G, sumsq, 0.0), raw_muon_step(values, quarter, MUON_G, sumsq, 2.0 ** 21)):
        for a, b in zip(today[0] + today[1], other[0] + other[1]):
            assert torch.equal(a, b)


def test_fused_muon_with_its_own_clip_equals_the_shared_one():
    """FusedMuon(max_grad_norm=) makes the norm pass over its own gradients: the same table, so the same bits, as a multi-optimizer
    that holds nothing else -- and not the unclipped step"""
    M = optim()
    gen = torch.Generator().manual_seed(37)
    init = [torch.randn(*s, generator=gen) * 0.1 for s in PROBE["MUON"]]
    a, b, c = device_params(init), device_params(init), device_params(init)
    own = M.FusedMuon(a, max_grad_norm=0.5, **MUON_G)
    multi = M.FusedMultiOptimizer({"MUON": M.FusedMuon(b, **MUON_G)}, max_grad_norm=0.5)
    plain = M.FusedMuon(c, **MUON_G)
    for s in range(2):
        grads = [torch.randn(*shape, generator=gen) for shape in PROBE["MUON"]]
        for ps in (a, b, c):
            for p, g in zip(ps, grads):
                set_grad(p, g)
        before = L.lib().lnx_optim_launches()
        own.step()
        assert L.lib().lnx_optim_launches() - before == 2
        multi.step()
        plain.step()
        want = sum(float(g.double().pow(2).sum()) for g in grads) ** 0.5
        np.testing.assert_allclose(float(own.grad_norm()), want, rtol=1e-5, atol=1e-6)
        assert torch.equal(own.grad_norm(), multi.grad_norm()) and plain.grad_norm() is None
        assert states_equal(own, a, multi.optimizers["MUON"], b)
        assert not torch.equal(own.state[a[0]]["momentum_buffer"], plain.state[c[0]]["momentum_buffer"])


# ------------------------------------------------------------------------------------------------------------------ union norm
UNION = {"MUON": [(48, 192), (33, 33)], "ADAMW": [(4097,), (33, 7)], "ADEMAMIX": [(1025,), (8193,)], "SGD": [(4096,), (5,)]}


def union_run(order, clip, seed=35, solo=False):
    gen = torch.Generator().manual_seed(seed)
    init = {k: [torch.randn(*s, generator=gen) * 0.1 for s in v] for k, v in UNION.items()}
    grads = {k: [torch.randn(*s, generator=gen) for s in v] for k, v in UNION.items()}
    params = {k: device_params(v) for k, v in init.items()}
    for k in UNION:
        for p, g in zip(params[k], grads[k]):
            set_grad(p, g)
    subs = {k: make_sub(k, params[k]) for k in order}
    if solo:
        for o in subs.values():
            o.step()
        return subs, params, grads, None
    multi = optim().FusedMultiOptimizer(subs, max_grad_norm=clip)
    multi.step()
    return subs, params, grads, multi.grad_norm().clone()


def test_union_norm_and_steps_under_the_clip():
    """The union table lists the parameters by sorted optimizer name, group, position: the per-workgroup partials and their fixed-order
    fold see the same sequence whatever order the optimizers were inserted in."""
    names = list(UNION)
    subs_a, params_a, grads, norm_a = union_run(names, 1e6)
    want = sum(float(g.double().pow(2).sum()) for v in grads.values() for g in v) ** 0.5
    np.testing.assert_allclose(float(norm_a), want, rtol=1e-5, atol=1e-6)
    _, _, _, norm_b = union_run(names, 1e6)
    subs_c, params_c, _, norm_c = union_run(names[::-1], 1e6)
    assert torch.equal(norm_a, norm_b) and torch.equal(norm_a, norm_c)
    # the norm is far under the clip: coef is 1 exactly and every sub-optimizer does what it does alone
    subs_s, params_s, _, _ = union_run(names, None, solo=True)
    for k in names:
        assert states_equal(subs_a[k], params_a[k], subs_s[k], params_s[k]), k
        assert states_equal(subs_c[k], params_c[k], subs_s[k], params_s[k]), k


# ------------------------------------------------------------------------------------------------------------------ the reference's steps
def test_replay_of_the_reference_steps(golden_dir):
    z = np.load(f"{golden_dir}/optim_step.npz")
    M = optim()
    clip, steps = float(z["clip"]), int(z["steps"])
    count = {"MUON": 2, "ADAMW": 2, "SGD": 2}
    params = {k: [torch.nn.Parameter(torch.from_numpy(z[f"{k}_{i}_init"]).cuda()) for i in range(n)] for k, n in count.items()}
    multi = M.FusedMultiOptimizer({"MUON": M.FusedMuon(params["MUON"], **MUON_G), "ADAMW": M.FusedAdamW(params["ADAMW"], **ADAMW_G),
                                   "SGD": M.FusedSGD(params["SGD"], **SGD_G)}, max_grad_norm=clip)
    muon = multi.optimizers["MUON"]
    big_muon = [torch.zeros(p.shape) for p in params["MUON"]]
    for s in range(steps):
        for k, ps in params.items():
            for i, p in enumerate(ps):
                set_grad(p, torch.from_numpy(z[f"{k}_{i}_grad{s}"]))
        before = [(p.detach().cpu(), muon.state[p]["momentum_buffer"].cpu() if p in muon.state else None) for p in params["MUON"]]
        multi.step()
        got = [float(v) for v in multi.grad_norms()]
        print(f"[replay] step {s}: norms {got}  reference {z['norms'][s].tolist()}")
        # the reference measures the clipped gradients again; here post = pre * coef: the same to fp32 rounding
        np.testing.assert_allclose(got, z["norms"][s], rtol=1e-5)
        assert (got[0] > clip) == (z["norms"][s, 0] > clip)
        for k in ("ADAMW", "SGD"):
            for i, p in enumerate(params[k]):
                torch.testing.assert_close(p.detach().cpu(), torch.from_numpy(z[f"{k}_{i}_after{s}"]), rtol=RTOL, atol=ATOL, msg=lambda m: f"{k} {i} step {s}: {m}")
        coef = np.float32(min(1.0, clip / (float(z["norms"][s, 0]) + 1e-6)))
        for i, p in enumerate(params["MUON"]):
            g = torch.from_numpy(z[f"MUON_{i}_grad{s}"]) * float(coef)  # the gradient Muon sees: after the clip
            big_muon[i] = torch.maximum(big_muon[i], g.abs())
            p_old, buf_old = before[i]
            u_hip = R.recover_update(p_old.double(), p.detach().cpu().double(), MUON_G)
            _, _, o_ref = R.step(p_old, g, buf_old, MUON_G)
            _, _, o_exact = R.step(p_old, g, buf_old, MUON_G, exact=True)
            e_ref, e_hip = (o_ref.double() - o_exact).abs().max().item(), (u_hip - o_exact).abs().max().item()
            d = (u_hip - o_ref.double()).abs().max().item()
            print(f"[replay] step {s} muon {i}: max|ref - exact| {e_ref:.4f}  max|hip - exact| {e_hip:.4f}  max|hip - ref| {d:.4f}")
            assert e_hip <= 1.5 * e_ref + 2e-3 and d <= 2.5 * e_ref + 4e-3, (s, i, e_hip, e_ref, d)
    for i, p in enumerate(params["MUON"]):
        got, want = muon.state[p]["momentum_buffer"].cpu(), torch.from_numpy(z[f"MUON_{i}_buf"])
        assert ((got - want).abs() <= 4 * 2.0 ** -23 * big_muon[i]).all(), i
    gmax = lambda k, i: max(float(np.abs(z[f"{k}_{i}_grad{s}"]).max()) for s in range(steps))  # noqa: E731  (before the clip: an upper bound of what entered)
    for i, p in enumerate(params["ADAMW"]):
        st = multi.optimizers["ADAMW"].state[p]
        assert int(st["step"]) == int(z[f"ADAMW_{i}_step"])
        torch.testing.assert_close(st["exp_avg"].cpu(), torch.from_numpy(z[f"ADAMW_{i}_exp_avg"]), rtol=RTOL, atol=ULP8 * gmax("ADAMW", i))
        torch.testing.assert_close(st["exp_avg_sq"].cpu(), torch.from_numpy(z[f"ADAMW_{i}_exp_avg_sq"]), rtol=RTOL, atol=ULP8 * gmax("ADAMW", i) ** 2)
    for i, p in enumerate(params["SGD"]):
        big = gmax("SGD", i) + SGD_G["weight_decay"] * float(np.abs(z[f"SGD_{i}_init"]).max())
        torch.testing.assert_close(multi.optimizers["SGD"].state[p]["momentum_buffer"].cpu(), torch.from_numpy(z[f"SGD_{i}_buf"]), rtol=RTOL, atol=ULP8 * big)
    # finding 2: the reference's own state_dict() of these optimizers saved no state; ours does
    assert not z["ref_state_dict_state_sizes"].any()
    assert [len(v["state"]) for v in multi.state_dict()["optimizers"].values()] == [2, 2, 2]


# ------------------------------------------------------------------------------------------------------------------ launches, no sync
@pytest.mark.parametrize("clip", [32.0, None], ids=["clipped", "unclipped"])
def test_launch_counts_and_no_host_synchronisation(clip):
    lib = L.lib()
    gen = torch.Generator().manual_seed(36)
    params = {k: device_params([torch.randn(*s, generator=gen) * 0.1 for s in v]) for k, v in UNION.items()}
    for ps in params.values():
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).cuda()
    multi = optim().FusedMultiOptimizer({k: make_sub(k, ps) for k, ps in params.items()}, max_grad_norm=clip)
    multi.step()  # builds and uploads every table (copies from pageable host memory synchronise)
    torch.cuda.synchronize()
    o0, m0 = lib.lnx_optim_launches(), lib.lnx_muon_launches()
    torch.cuda.set_sync_debug_mode("error")
    try:
        multi.step()
        multi.step()
        norms = multi.grad_norms()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert lib.lnx_optim_launches() - o0 == 2 * ((2 if clip else 0) + 3)  # the norm pass, then AdamW, AdEMAMix and SGD one launch each
    assert lib.lnx_muon_launches() - m0 == 2 * (3 * MUON_G["ns_steps"] + 3)
    assert (norms is None) == (clip is None)
    if clip:
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.ndim == 0 for v in norms)
    assert all(torch.isfinite(p).all() for ps in params.values() for p in ps)


# ------------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("freeze", [False, True], ids=["trained", "freeze_4d_like_reference"])
def test_build_optimizer_trains_the_tiny_model(golden_dir, freeze):
    from linnaeus_amd.loss import multitask_cross_entropy
    from tests.cases import load_train_step
    from tests.test_gpu_model import build

    spec, z, sd, x, meta, targets, weights = load_train_step(golden_dir)
    model = build("tiny_a", spec, sd, "fp32")
    model.train()
    model.grad_mode = "direct"
    xg, mg = x.cuda(), meta.cuda()
    tg = {t: v.cuda() for t, v in targets.items()}
    cfg = ConfigNode({"OPTIMIZER": {"NAME": "muon"}, "LR_SCHEDULER": {"BASE_LR": 1e-3}, "TRAIN": {"CLIP_GRAD": 1.0}})
    opt = optim().build_optimizer(cfg, model, freeze_4d_like_reference=freeze)
    assert type(opt).__name__ == "FusedMultiOptimizer" and list(opt.optimizers) == ["MUON", "ADAMW"] and opt.max_grad_norm == 1.0
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    had_grad = set()
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        multitask_cross_entropy(model(xg, mg), tg, weights).backward()
        had_grad |= {n for n, p in model.named_parameters() if p.grad is not None}
        opt.step()
    assert float(opt.grad_norm()) > 0
    four_d = [n for n, p in model.named_parameters() if p.dim() == 4]
    assert four_d and set(four_d) <= had_grad
    for n, p in model.named_parameters():
        assert torch.isfinite(p).all(), n
        if freeze and p.dim() == 4:
            assert torch.equal(p.detach(), start[n]), n  # what the reference does to a conv weight it hands to Muon
        elif n in had_grad:
            assert not torch.equal(p.detach(), start[n]), n
