"""The abstention kernels on the GPU (include/lnx.h: lnx_abstain_act, lnx_ppo_advantages, lnx_ppo_loss_fwd / _bwd) against the fp64
restatement of tests/abstention_ref.py, and linnaeus_amd/rl.py end to end on the tiny model.

Shapes.  The class counts {1, 2, 63, 64, 65, 255, 257, 1023, 1025, 10 007} sit below, at and above a wave (64), the workgroup (256: where
a thread's chunk grows from one class to two) and four workgroups; they are spread over the ranks of five cases (a rank has its own C)
that also cover B in {1, 3, 257}, R in {1, 4, 8}, ld = C and ld = C + 5 (padding columns hold NaN: a read of one would spoil the row),
fp32 and bf16 (the restatement is fed the rounded values).  Every case has a row with one logit 200 above the rest and a row of
all-equal logits where B allows, and targets with a null at every rank position.

Tolerances are those of tests/test_loss.py on the GPU: rtol 2e-5 / atol 2e-6 for values, rtol 2e-4 / atol 2e-6 for gradients.

Sampled actions equal the fp64 inverse CDF exactly wherever u lies more than 1e-5 from both boundaries of the restatement's class; on
the other rows the action is that class or a neighbour, and those rows are at most 1 % of a case's rows.  The seeds below were chosen
on the CPU so that the restatement alone meets that bound (the test asserts it again); the large heads are peaked (a class boosted by
log C + 6) because a flat 10 007-class row has a fifth of [0, 1) within 1e-5 of a boundary.

Launches (the bar of the issue): 1 for act, 1 for advantages, 2 + 1 for the loss, asserted through lnx_abstain_launches."""
import math

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import rl
from tests import abstention_ref as R

pytestmark = pytest.mark.gpu
VAL = dict(rtol=2e-5, atol=2e-6)
GRAD = dict(rtol=2e-4, atol=2e-6)
REWARDS = [("simple", "all"), ("simple", "first"), ("outcome", "all"), ("outcome", "first")]

CASES = {
    # name: B, class counts in decision order, padding columns, dtype, seed
    "wide8": dict(B=257, Cs=[1023, 257, 255, 65, 64, 63, 2, 1], pad=0, dtype=torch.float32, seed=1),
    "wide8_pad": dict(B=3, Cs=[1023, 257, 255, 65, 64, 63, 2, 1], pad=5, dtype=torch.bfloat16, seed=1),
    "big4": dict(B=257, Cs=[1025, 10007, 64, 255], pad=5, dtype=torch.bfloat16, seed=2),
    "big4_f32": dict(B=3, Cs=[10007, 1025, 2, 65], pad=0, dtype=torch.float32, seed=1),
    "one": dict(B=1, Cs=[10007], pad=5, dtype=torch.float32, seed=1),
}
_PROBLEMS = {}
_REFS = {}


def make_problem(name):
    """CPU tensors: padded logits [B, C + pad] per rank (NaN in the padding), targets, uniforms, abstain / null indices"""
    if name in _PROBLEMS:
        return _PROBLEMS[name]
    c = CASES[name]
    B, Cs, pad, dtype = c["B"], c["Cs"], c["pad"], c["dtype"]
    g = torch.Generator().manual_seed(1000 + c["seed"])
    padded, targets, abstain, null = [], [], [], []
    for r, C_ in enumerate(Cs):
        x = torch.randn(B, C_, generator=g) * 2.0
        boost = math.log(C_) + 6.0 if C_ > 300 else 3.0
        true = torch.randint(0, C_, (B,), generator=g)
        x[torch.arange(B), true] += boost
        ab = 1 if (r % 2 == 1 and C_ >= 3) else 0  # (odd ranks: an abstain class other than 0)
        nl = 2 if (r % 2 == 1 and C_ >= 3) else 0
        # every other row: the abstain class gets a probability of about 0.2, so that sequential episodes end at every rank
        if C_ > 1:
            others = x.clone()
            others[:, ab] = -float("inf")
            x[::2, ab] = (torch.logsumexp(others, dim=1) + math.log(0.25))[::2]
        if B >= 3:
            x[1] = torch.randn(C_, generator=g)
            x[1, int(true[1])] += 200.0  # one logit 200 above the rest
            x[2] = 0.75                  # all equal
        t = torch.where(torch.rand(B, generator=g) < 0.6, true, torch.randint(0, C_, (B,), generator=g))
        t[torch.rand(B, generator=g) < 0.3] = nl
        t[r % B] = nl  # a null at every rank position
        full = torch.full((B, C_ + pad), float("nan"))
        full[:, :C_] = x
        padded.append(full.to(dtype))
        targets.append(t)
        abstain.append(ab)
        null.append(nl)
    u = torch.rand(B, len(Cs), generator=g)
    _PROBLEMS[name] = (padded, targets, u, abstain, null)
    return _PROBLEMS[name]


def views(padded, Cs):
    return [p[:, :C_] for p, C_ in zip(padded, Cs)]


def on_gpu(name):
    padded, targets, u, abstain, null = make_problem(name)
    Cs = CASES[name]["Cs"]
    return views([p.cuda() for p in padded], Cs), [t.cuda() for t in targets], u.cuda()


def cpu_logits(name):
    return [v.float() for v in views(make_problem(name)[0], CASES[name]["Cs"])]


def own_reference(name):
    """the restatement's own draw, once per case (shared, never modified)"""
    if name not in _REFS:
        _, targets, u, abstain, null = make_problem(name)
        _REFS[name] = R.rollout_ref(cpu_logits(name), targets, u, "multitask", abstain=abstain, null=null)
    return _REFS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_seeds_meet_the_boundary_bound_on_the_reference_alone(name):
    near = own_reference(name)["margin"] <= 1e-5
    assert near.sum().item() <= 0.01 * near.numel(), (int(near.sum()), near.numel())


@pytest.mark.parametrize("mode", ["multitask", "sequential"])
@pytest.mark.parametrize("name", list(CASES))
def test_act_against_fp64(name, mode):
    padded, targets, u, abstain, null = make_problem(name)
    Cs = CASES[name]["Cs"]
    logits, tg, ud = on_gpu(name)
    lib = L.lib()
    first = None
    for kind, ranks in REWARDS:
        counts = rl.new_counts("cuda")
        before = lib.lnx_abstain_launches()
        got = rl.act(logits, tg, ud, mode, False, rl.AbstentionReward(kind, ranks), abstain, null, counts)
        assert lib.lnx_abstain_launches() - before == 1
        got = rl.Acted(*[t.cpu() for t in got])
        ref = R.rollout_ref(cpu_logits(name), targets, u, mode, kind=kind, ranks=ranks, abstain=abstain, null=null, forced_actions=got.actions)
        assert torch.equal(got.reward.double(), ref["reward"]), (kind, ranks)  # dyadic tables: exact sums
        assert counts.cpu().tolist() == ref["counts"], (kind, ranks)
        if first is not None:  # the decisions do not depend on the reward
            assert all(torch.equal(a, b) for a, b in zip(got[:5], first[:5]))
            continue
        first = got
        own = own_reference(name)
        tk = got.taken.bool()
        far = (own["margin"] > 1e-5) & tk
        assert torch.equal(got.actions.long()[far], own["own_actions"][far])
        near = ~(own["margin"] > 1e-5) & tk
        assert ((got.actions.long() - own["own_actions"]).abs()[near] <= 1).all()
        assert near.sum().item() <= 0.01 * near.numel()
        for r, C_ in enumerate(Cs):
            assert int(got.actions[:, r].min()) >= 0 and int(got.actions[:, r].max()) < C_
        assert torch.equal(got.taken, ref["taken"]) and torch.equal(got.length, ref["length"])
        assert torch.equal(got.actions.long(), ref["actions"])  # untaken ranks report the abstain index
        print(name, mode, "logp err", float((got.logp.double() - ref["logp"]).abs().max()), "H err", float((got.entropy.double() - ref["entropy"]).abs().max()))
        torch.testing.assert_close(got.logp.double(), ref["logp"], **VAL)
        torch.testing.assert_close(got.entropy.double(), ref["entropy"], **VAL)
        if mode == "sequential" and len(Cs) > 1 and CASES[name]["B"] > 100:
            assert set(got.length.tolist()) == set(range(1, len(Cs) + 1))  # episodes of every length
        else:
            assert mode == "sequential" or bool(tk.all())


@pytest.mark.parametrize("name", list(CASES))
def test_greedy_is_the_lowest_arg_max_and_needs_no_u(name):
    padded, targets, u, abstain, null = make_problem(name)
    logits, tg, _ = on_gpu(name)
    got = rl.act(logits, tg, None, "sequential", True, None, abstain, null)
    ref = R.rollout_ref(cpu_logits(name), targets, None, "sequential", greedy=True, abstain=abstain, null=null)
    assert torch.equal(got.actions.cpu().long(), ref["actions"]) and torch.equal(got.taken.cpu(), ref["taken"])
    multi = rl.act(logits, tg, None, "multitask", True, None, abstain, null)
    assert torch.equal(multi.actions.cpu().long(), ref["greedy"])
    if CASES[name]["B"] >= 3:
        assert [int(v) for v in multi.actions[2].cpu()] == [0] * len(logits)  # the all-equal row: the lowest index
    torch.testing.assert_close(multi.logp.cpu().double(), R.rollout_ref(cpu_logits(name), targets, None, "multitask", greedy=True, abstain=abstain,
                                                                        null=null)["logp"], **VAL)


@pytest.mark.parametrize("mode", ["multitask", "sequential"])
@pytest.mark.parametrize("name", ["wide8", "big4", "one"])
def test_advantages_against_fp64_and_bit_identical(name, mode):
    _, _, _, abstain, null = make_problem(name)
    logits, tg, ud = on_gpu(name)
    Rn, B = len(logits), CASES[name]["B"]
    got = rl.act(logits, tg, ud, mode, False, rl.AbstentionReward("simple", "all"), abstain, null)
    value = torch.randn(B, generator=torch.Generator().manual_seed(77)).cuda()
    lib = L.lib()
    before = lib.lnx_abstain_launches()
    adv, ret, n = rl.advantages(got.reward, value, got.length, mode, Rn, 0.99, 0.95)
    assert lib.lnx_abstain_launches() - before == 1
    adv2, ret2, n2 = rl.advantages(got.reward, value, got.length, mode, Rn, 0.99, 0.95)
    assert torch.equal(adv, adv2) and torch.equal(ret, ret2) and torch.equal(n, n2)  # the same bits run to run
    adv_ref, ret_ref, n_ref = R.advantages_ref(got.reward.cpu().numpy(), value.cpu().numpy(), got.length.cpu().numpy(), mode, Rn, 0.99, 0.95)
    assert int(n) == n_ref == (int(got.length.sum()) if mode == "sequential" else B)
    print(name, mode, "adv err", float((adv.cpu().double() - adv_ref).abs().max()), "ret err", float((ret.cpu().double() - ret_ref).abs().max()))
    torch.testing.assert_close(adv.cpu().double(), adv_ref, **VAL)
    torch.testing.assert_close(ret.cpu().double(), ret_ref, **VAL)


def loss_inputs(name, mode, variant):
    """the rollout of the case, its advantages, and logp_old: the rollout's own (ratio = 1 exactly) or placed so that the ratios sit
    1e-3 inside and outside 1 - eps and 1 + eps (both signs of A occur among the normalised advantages)"""
    _, _, _, abstain, null = make_problem(name)
    logits, tg, ud = on_gpu(name)
    B, Rn = CASES[name]["B"], len(logits)
    got = rl.act(logits, tg, ud, mode, False, rl.AbstentionReward("simple", "all"), abstain, null)
    value = torch.randn(B, generator=torch.Generator().manual_seed(78)).cuda()
    adv, ret, _ = rl.advantages(got.reward, value, got.length, mode, Rn, 0.99, 0.95)
    logp_old = got.logp.clone()
    if variant == "edges":
        ratios = torch.tensor([0.8 - 1e-3, 0.8 + 1e-3, 1.2 - 1e-3, 1.2 + 1e-3, 1.0, 0.5, 1.7])
        pick = ratios[torch.arange(B * Rn).reshape(B, Rn) % len(ratios)].cuda()
        if mode == "multitask":  # the ratio of a sample is the product over its ranks: move rank 0 only
            pick = torch.cat([pick[:, :1], torch.ones(B, Rn - 1).cuda()], dim=1)
        logp_old = (got.logp.double() - torch.log(pick.double())).float() * got.taken
    return logits, got, value, adv, ret, logp_old


@pytest.mark.parametrize("variant", ["same", "edges"])
@pytest.mark.parametrize("mode", ["multitask", "sequential"])
@pytest.mark.parametrize("name", ["wide8", "wide8_pad", "big4", "big4_f32", "one"])
def test_loss_and_gradients_against_fp64_autograd(name, mode, variant):
    logits, got, value, adv, ret, logp_old = loss_inputs(name, mode, variant)
    Cs, pad, B = CASES[name]["Cs"], CASES[name]["pad"], CASES[name]["B"]
    lib = L.lib()
    before = lib.lnx_abstain_launches()
    args, out = rl.loss_forward(logits, value, got.actions, got.taken, logp_old, adv, ret, mode, 0.2, 0.5, 0.01)
    assert lib.lnx_abstain_launches() - before == 2
    SENT = -123.5
    dl = [torch.full((B, C_ + pad), SENT, device="cuda") for C_ in Cs]
    dv = torch.full((B,), SENT, device="cuda")
    go = torch.tensor([1.25], device="cuda")
    rl.loss_backward(args, go, views(dl, Cs), dv)
    assert lib.lnx_abstain_launches() - before == 3

    cpu = [v.float() for v in views(make_problem(name)[0], Cs)]
    want, dl_ref, dv_ref = R.ppo_loss_ref(cpu, value.cpu(), got.actions.cpu(), got.taken.cpu(), logp_old.cpu(), adv.cpu(), ret.cpu(), mode, 0.2, 0.5, 0.01)
    out = out.cpu()
    names = ("policy_loss", "value_loss", "entropy_loss", "total_loss", "n", "ratio_mean", "clip_frac")
    print(name, mode, variant, {k: (float(out[i]), want[k]) for i, k in enumerate(names)})
    for i, k in enumerate(names):
        torch.testing.assert_close(float(out[i]), want[k], **VAL)
    if variant == "same":
        assert float(out[L.PPO_OUT_RATIO_MEAN]) == 1.0 and float(out[L.PPO_OUT_CLIP_FRAC]) == 0.0  # ratio = 1 exactly: the same bits as the rollout
    elif B > 100:
        assert 0.2 < want["clip_frac"] < 0.9
    taken = got.taken.cpu().bool()
    for r, C_ in enumerate(Cs):
        d = dl[r].cpu()
        assert bool((d[:, C_:] == SENT).all())  # the padding columns come back untouched
        rows = taken[:, r] if mode == "sequential" else torch.ones(B, dtype=torch.bool)
        assert bool((d[~rows, :C_] == SENT).all())  # and so do the rows of untaken ranks
        torch.testing.assert_close(d[rows, :C_].double(), 1.25 * dl_ref[r][rows], **GRAD)
    torch.testing.assert_close(dv.cpu().double(), 1.25 * dv_ref, **GRAD)
    if variant == "same":  # d/dratio = A at ratio = 1: the gradient of -mean(A logp) alone, without the entropy term
        args0, _ = rl.loss_forward(logits, value, got.actions, got.taken, logp_old, adv, ret, mode, 0.2, 0.5, 0.0)
        d0 = [torch.zeros(B, C_, device="cuda") for C_ in Cs]
        rl.loss_backward(args0, torch.ones(1, device="cuda"), d0, None)
        n = float(out[L.PPO_OUT_N])
        for r, C_ in enumerate(Cs):
            z = cpu[r].double()
            p = torch.softmax(z, dim=1)
            onehot = torch.nn.functional.one_hot(got.actions[:, r].cpu().long(), C_).double()
            A = (adv[:, r] if mode == "sequential" else adv[:, 0]).cpu().double()
            rows = taken[:, r] if mode == "sequential" else torch.ones(B, dtype=torch.bool)
            torch.testing.assert_close(d0[r].cpu().double()[rows], (-(A / n)[:, None] * (onehot - p))[rows], **GRAD)


def test_autograd_function_matches_the_raw_calls():
    logits, got, value, adv, ret, logp_old = loss_inputs("wide8_pad", "sequential", "edges")
    lg = [x.detach().float().clone().requires_grad_(True) for x in logits]
    v = value.clone().requires_grad_(True)
    total, stats = rl.ppo_loss(lg, v, got.actions, got.taken, logp_old, adv, ret, "sequential", 0.2, 0.5, 0.01)
    (2.0 * total).backward()
    cpu = [x.detach().cpu() for x in lg]
    want, dl_ref, dv_ref = R.ppo_loss_ref(cpu, value.cpu(), got.actions.cpu(), got.taken.cpu(), logp_old.cpu(), adv.cpu(), ret.cpu(), "sequential")
    torch.testing.assert_close(total.item(), want["total_loss"], **VAL)
    torch.testing.assert_close(float(stats["policy_loss"]), want["policy_loss"], **VAL)
    for x, d in zip(lg, dl_ref):
        torch.testing.assert_close(x.grad.cpu().double(), 2.0 * d, **GRAD)
    torch.testing.assert_close(v.grad.cpu().double(), 2.0 * dv_ref, **GRAD)


# ------------------------------------------------------------------------------------------------------------------ end to end
# aggregate.bias is ONE scalar added to every feature in front of final_norm, and a LayerNorm does not see a shift of all its inputs:
# the gradient of this parameter is 0 in exact arithmetic under any loss (what arrives is rounding, measured 7e-9 and 6e-8 here against
# 1e-2 .. 1 for every other parameter).  It is asserted finite and negligible; every other parameter must get a non-zero gradient.
SHIFT_ONLY = {"model.aggregate.bias"}
def tiny_policy(golden_dir, mode):
    from linnaeus_amd import build_model
    from tests.cases import CASES as MODELS, load_case, make_config, model_state_dict_from_oracle

    spec, z, sd, x, meta, drops = load_case("tiny_c", golden_dir)
    model = build_model(make_config(spec, 64), num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda().train()
    model.set_compute_dtype("fp32")
    torch.manual_seed(3)
    policy = rl.AbstentionPolicy(model, mode).cuda()
    g = torch.Generator().manual_seed(9)
    images = torch.randn(8, 3, 64, 64, generator=g).cuda()
    targets = {t: torch.randint(0, c, (8,), generator=g).cuda() for t, c in spec.heads}
    u = torch.rand(8, len(spec.heads), generator=g)
    u[:4] = 0.9 + 0.1 * u[:4]  # class 0, the abstain class, comes first in the running sum: these samples reach the last rank
    return policy, images, targets, u.cuda()


def one_update(golden_dir, mode, monkeypatch, fused):
    monkeypatch.setenv("LNX_ABSTENTION", "1" if fused else "0")
    policy, images, targets, u = tiny_policy(golden_dir, mode)
    assert policy.rank_order == ["taxa_L30", "taxa_L20", "taxa_L10"]  # coarsest first
    batch = rl.rollout(policy, images, None, targets, reward=rl.AbstentionReward("simple", "all"), u=u)
    opt = torch.optim.SGD(policy.parameters(), lr=0.0)  # lr 0: the gradients stay in .grad and the parameters where they were
    stats = rl.ppo_update(policy, opt, batch, ppo_epochs=1, minibatch=8, max_grad_norm=0.0)
    grads = {n: p.grad.detach().cpu().clone() for n, p in policy.named_parameters() if p.requires_grad}
    return batch, {k: float(v) for k, v in stats.items()}, grads


@pytest.mark.parametrize("mode", ["multitask", "sequential"])
def test_rollout_and_update_on_the_tiny_model(golden_dir, monkeypatch, mode):
    lib = L.lib()
    before = lib.lnx_abstain_launches()
    batch, stats, grads = one_update(golden_dir, mode, monkeypatch, fused=True)
    assert lib.lnx_abstain_launches() - before == 1 + 1 + 2 + 1  # act, advantages, loss forward, loss backward
    assert any(n.startswith("value_head") for n in grads)
    for n, g in grads.items():
        assert torch.isfinite(g).all(), n
        if n in SHIFT_ONLY:
            assert float(g.abs().max()) < 1e-6, n
        else:
            assert float(g.abs().max()) > 0.0, n
    before = lib.lnx_abstain_launches()
    batch0, stats0, grads0 = one_update(golden_dir, mode, monkeypatch, fused=False)
    assert lib.lnx_abstain_launches() == before  # LNX_ABSTENTION=0: the torch composition, no launch
    assert torch.equal(batch.acted.actions, batch0.acted.actions) and torch.equal(batch.acted.length, batch0.acted.length)
    assert torch.equal(batch.acted.reward, batch0.acted.reward)
    torch.testing.assert_close(batch.adv, batch0.adv, **VAL)
    print(mode, stats, stats0)
    for k in stats:
        torch.testing.assert_close(stats[k], stats0[k], **VAL)
    for n in grads:
        print(n, "grad err", float((grads[n] - grads0[n]).abs().max()), "of", float(grads0[n].abs().max()))
    for n in grads:
        torch.testing.assert_close(grads[n], grads0[n], **GRAD)


@pytest.mark.parametrize("mode", ["multitask", "sequential"])
def test_evaluate_policy_equals_the_restatement(golden_dir, monkeypatch, mode):
    monkeypatch.setenv("LNX_ABSTENTION", "1")
    policy, images, targets, _ = tiny_policy(golden_dir, mode)
    loader = [(images[:5], None, {t: v[:5] for t, v in targets.items()}), (images[5:], None, {t: v[5:] for t, v in targets.items()})]
    res, counts = rl.evaluate_policy(policy, loader, rl.AbstentionReward("simple", "all"), return_counts=True)
    policy.eval()
    with torch.no_grad():
        logits, _ = policy(images, None)
    ref = R.rollout_ref([x.float().cpu() for x in logits], [targets[t].cpu() for t in policy.rank_order], None, mode, greedy=True)
    assert counts == ref["counts"]
    assert res["mean_reward"] == float(ref["reward"].mean()) and res["median_reward"] == float(ref["reward"].quantile(0.5))
    assert res["mean_length"] == float(ref["length"].double().mean())
    c = dict(zip(R.COUNTERS, ref["counts"][:7]))
    assert res["abst_rate/taxa_L30"] == c["abstained"] / 8
    assert res["missed_abst_count/taxa_L30"] == c["missed_abstain"]
    for key in ("abst_rate", "corr_abst_rate", "unnec_abst_rate", "recall_abst", "acc_on_non_abst", "missed_abst_count"):
        assert all(f"{key}/{t}" in res for t in policy.rank_order)


def test_update_steps_with_the_fused_adamw_and_its_clip(golden_dir, monkeypatch):
    """minibatches of 4 out of 8 samples (shuffled on the device), two epochs, FusedAdamW clipping inside its step: three launches per
    step with the clip, `max_grad_norm` set for the update only"""
    from linnaeus_amd.optim import FusedAdamW

    monkeypatch.setenv("LNX_ABSTENTION", "1")
    policy, images, targets, u = tiny_policy(golden_dir, "sequential")
    start = {n: p.detach().clone() for n, p in policy.named_parameters()}
    opt = FusedAdamW(policy.parameters(), lr=1e-3)
    batch = rl.rollout(policy, images, None, targets, u=u)
    lib = L.lib()
    steps_before, launches_before = lib.lnx_optim_launches(), lib.lnx_abstain_launches()
    stats = rl.ppo_update(policy, opt, batch, ppo_epochs=2, minibatch=4, max_grad_norm=0.5, generator=torch.Generator(device="cuda").manual_seed(1))
    assert lib.lnx_optim_launches() - steps_before == 2 * 2 * 3
    assert lib.lnx_abstain_launches() - launches_before == 2 * 2 * 3
    assert opt.max_grad_norm is None
    assert all(math.isfinite(float(v)) for v in stats.values()) and float(stats["n"]) >= 4
    for n, p in policy.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), start[n]), n
