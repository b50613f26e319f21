"""The abstention phase on the device: batched rollout, rewards, advantages and the PPO loss in HIP.

The reference's phase 2 (rl_train_abstention.py, rl_env/) trains a policy that may answer "abstain" at a taxonomic rank.  A decision at
rank r depends on the image only, so a whole episode in either mode follows from ONE forward pass; what comes after the forward is
row-wise work over [B, C] logits, done here in a fixed number of launches (include/lnx.h: lnx_abstain_act, lnx_ppo_advantages,
lnx_ppo_loss_fwd / lnx_ppo_loss_bwd):

    policy = AbstentionPolicy(model, mode="sequential")
    batch = rollout(policy, images, meta, targets, reward=AbstentionReward("simple"))     # 1 forward + 2 launches, no host read
    stats = ppo_update(policy, optimizer, batch, ppo_epochs=4, minibatch=64)              # per minibatch: 1 forward, 3 launches, 1 backward
    results = evaluate_policy(policy, loader)                                             # one read-back at the end

`LNX_ABSTENTION=0`, read per call, runs a torch composition of the same definitions instead (fp32, any device); the functions `act`,
`advantages` and `ppo_loss` below take plain tensors and are what the tests and tools/bench_abstention.py drive.

What differs from the reference is listed in INTEGRATION.md ("Abstention phase on device", findings F-a to F-d).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
import torch.nn as nn

from . import _lib as L

MODES = {"multitask": L.ABSTAIN_MULTITASK, "sequential": L.ABSTAIN_SEQUENTIAL}
# the per-rank counters of the reference's evaluate_policy, in the order of the LNX_ABSTAIN_CNT_* enum
COUNTERS = ("abstained", "total_decisions", "correct_abstain", "unnecessary_abstain", "missed_abstain", "correct_classify_non_abstain",
            "misclassify_non_abstain")


def abstention_on_device() -> bool:
    """LNX_ABSTENTION=0 (read per call): the torch composition instead of the HIP kernels"""
    return os.environ.get("LNX_ABSTENTION", "1") != "0"


def launches() -> int:
    """kernel launches made by the four entry points since the library was loaded (lnx_abstain_launches)"""
    return int(L.lib().lnx_abstain_launches())


class AbstentionReward:
    """SimpleAbstentionReward (kind="simple": a table entry per counted rank, summed) or EpisodeOutcomeReward (kind="outcome": one value
    for the whole episode) of rl_env/reward_functions.py.  ranks="all" counts every rank, the list form the reference's docstrings
    describe; ranks="first" counts the first rank of the decision order only, which is what the reference's environment computes
    (finding F-a).  The keyword names are the reference's."""

    def __init__(self, kind: str = "simple", ranks: str = "all", reward_correct_classification: float = 1.0, reward_correct_abstention: float = 0.5,
                 penalty_misclassification: float = -1.0, penalty_unnecessary_abstention: float = -0.5,
                 penalty_incorrect_prediction_at_null_rank: float = -1.0, reward_optimal_outcome: float = 1.0, penalty_suboptimal_outcome: float = -1.0):
        if kind not in ("simple", "outcome"):
            raise ValueError(f"AbstentionReward: kind={kind!r} (simple or outcome)")
        if ranks not in ("all", "first"):
            raise ValueError(f"AbstentionReward: ranks={ranks!r} (all or first)")
        self.kind, self.ranks = kind, ranks
        # in the order of the LNX_ABSTAIN_* outcome enum
        self.table = [float(reward_correct_classification), float(reward_correct_abstention), float(penalty_misclassification),
                      float(penalty_unnecessary_abstention), float(penalty_incorrect_prediction_at_null_rank)]
        self.outcome = [float(reward_optimal_outcome), float(penalty_suboptimal_outcome)]

    @property
    def kind_code(self) -> int:
        return L.ABSTAIN_REWARD_SIMPLE if self.kind == "simple" else L.ABSTAIN_REWARD_OUTCOME

    @property
    def ranks_code(self) -> int:
        return L.ABSTAIN_RANKS_ALL if self.ranks == "all" else L.ABSTAIN_RANKS_FIRST


class Acted(NamedTuple):
    """what lnx_abstain_act writes: per decision [B, R] and per episode [B]"""
    actions: torch.Tensor  # int32 [B, R]
    logp: torch.Tensor     # fp32 [B, R]
    entropy: torch.Tensor  # fp32 [B, R]
    taken: torch.Tensor    # uint8 [B, R]
    length: torch.Tensor   # int32 [B]
    reward: torch.Tensor   # fp32 [B]


def new_counts(device) -> torch.Tensor:
    """an empty counter table for `act(..., counts=)` (int64 [LNX_ABSTAIN_COUNTS], layout in include/lnx.h)"""
    return torch.zeros(L.ABSTAIN_COUNTS, dtype=torch.int64, device=device)


def _mode_code(mode) -> int:
    if mode in MODES:
        return MODES[mode]
    if mode in MODES.values():
        return int(mode)
    raise ValueError(f"mode={mode!r} (multitask or sequential)")


def _per_rank(v, R: int, what: str) -> List[int]:
    out = [int(v)] * R if isinstance(v, int) else [int(x) for x in v]
    if len(out) != R:
        raise ValueError(f"{what}: {len(out)} values for {R} ranks")
    return out


def _stream(dev) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _prep_logits(logits: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """row views as they come (a padded leading dimension is the kernels' ld); only another dtype or strided columns cost a copy"""
    if not 1 <= len(logits) <= L.METRICS_MAX_TASKS:
        raise L.LnxError(f"abstention: {len(logits)} ranks (1..{L.METRICS_MAX_TASKS})")
    out = [x.detach() for x in logits]
    first = out[0]
    for i, x in enumerate(out):
        if x.dim() != 2 or x.shape[0] != first.shape[0]:
            raise L.LnxError(f"abstention: rank {i} has logits of shape {tuple(x.shape)}, batch {first.shape[0]}")
        if x.dtype != first.dtype or x.dtype not in (torch.float32, torch.bfloat16):
            out[i] = x = x.float() if first.dtype != torch.bfloat16 else x.to(torch.bfloat16)
        if (x.shape[1] > 1 and x.stride(1) != 1) or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
            out[i] = x.contiguous()
    return out


def _fill_ranks(rank, logits, abstain=None, null=None, targets=None) -> None:
    for r, x in enumerate(logits):
        k = rank[r]
        k.logits, k.ld, k.C = x.data_ptr(), (x.stride(0) if x.shape[0] > 1 else x.shape[1]), x.shape[1]
        if abstain is not None:
            k.abstain_index, k.null_index, k.target = abstain[r], null[r], targets[r].data_ptr()


# ------------------------------------------------------------------------------------------------------------------ rollout
def act(logits: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], u: Optional[torch.Tensor], mode="sequential", greedy: bool = False,
        reward: Optional[AbstentionReward] = None, abstain_index=0, null_index=0, counts: Optional[torch.Tensor] = None) -> Acted:
    """One rollout step for a batch: logits / targets per rank in DECISION order ([B, C_r] fp32 or bf16 row views, int64 [B]); u: [B, R]
    uniforms in [0, 1) (None with greedy).  counts: a `new_counts` table this batch is added to.  ONE launch, no host read."""
    reward = reward or AbstentionReward()
    R = len(logits)
    abstain, null = _per_rank(abstain_index, R, "abstain_index"), _per_rank(null_index, R, "null_index")
    if not abstention_on_device():
        return _act_torch(logits, targets, u, _mode_code(mode), greedy, reward, abstain, null, counts)
    xs = _prep_logits(logits)
    B, dev = xs[0].shape[0], xs[0].device
    if not xs[0].is_cuda:
        raise L.LnxError("abstention: the HIP kernels need the logits on the GPU (LNX_ABSTENTION=0 selects the torch composition)")
    tg = [t.to(device=dev, dtype=torch.int64).contiguous() for t in targets]
    if len(tg) != R or any(t.shape != (B,) for t in tg):
        raise L.LnxError(f"abstention: targets must be {R} tensors of shape [{B}]")
    if u is not None:
        u = u.to(device=dev, dtype=torch.float32).contiguous()
        if u.shape != (B, R):
            raise L.LnxError(f"abstention: u must be [{B}, {R}], got {tuple(u.shape)}")
    out = Acted(torch.empty(B, R, dtype=torch.int32, device=dev), torch.empty(B, R, device=dev), torch.empty(B, R, device=dev),
                torch.empty(B, R, dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, device=dev))
    a = L.AbstainActArgs()
    a.dtype, a.B, a.R, a.mode, a.greedy = (L.BF16 if xs[0].dtype == torch.bfloat16 else L.F32), B, R, _mode_code(mode), int(bool(greedy))
    a.reward_kind, a.reward_ranks = reward.kind_code, reward.ranks_code
    a.table[:] = reward.table
    a.outcome_reward[:] = reward.outcome
    a.u = None if u is None else u.data_ptr()
    a.actions, a.logp, a.entropy, a.taken = out.actions.data_ptr(), out.logp.data_ptr(), out.entropy.data_ptr(), out.taken.data_ptr()
    a.length, a.reward = out.length.data_ptr(), out.reward.data_ptr()
    if counts is not None:
        if counts.dtype != torch.int64 or counts.numel() != L.ABSTAIN_COUNTS or counts.device != dev or not counts.is_contiguous():
            raise L.LnxError(f"abstention: counts must be a contiguous int64 [{L.ABSTAIN_COUNTS}] tensor on {dev}")
        a.counts = counts.data_ptr()
    _fill_ranks(a.rank, xs, abstain, null, tg)
    L.check(L.lib().lnx_abstain_act(C.byref(a), _stream(dev)), "lnx_abstain_act")
    return out


def _first_index(cond: torch.Tensor) -> torch.Tensor:
    """per row the lowest column where cond holds, the column count where none does"""
    n = cond.shape[1]
    idx = torch.arange(n, device=cond.device).expand_as(cond)
    return torch.where(cond, idx, torch.full_like(idx, n)).min(dim=1).values


def _row_terms(x: torch.Tensor):
    """(z - max, exp of it, running sum, log of the total, arg-max with the lowest index on a tie) of fp32 rows"""
    z = x.float()
    mx = z.max(dim=1, keepdim=True).values
    d = z - mx
    e = torch.exp(d)
    cum = torch.cumsum(e, dim=1)
    return d, e, cum, torch.log(cum[:, -1]), _first_index(z == mx)


def _act_torch(logits, targets, u, mode, greedy, reward, abstain, null, counts) -> Acted:
    R, B, dev = len(logits), logits[0].shape[0], logits[0].device
    seq = mode == L.ABSTAIN_SEQUENTIAL
    stopped = torch.zeros(B, dtype=torch.bool, device=dev)
    length = torch.full((B,), R if seq else 1, dtype=torch.int32, device=dev)
    acts, logps, ents, takens, outcomes = [], [], [], [], []
    for r in range(R):
        d, e, cum, log_total, arg = _row_terms(logits[r])
        total = cum[:, -1]
        H = log_total - torch.where(e > 0, e * d, torch.zeros_like(e)).sum(dim=1) / total
        if greedy:
            a = arg
        else:
            j = _first_index(cum > (u[:, r].float().to(dev) * total)[:, None])
            a = torch.where(j < d.shape[1], j, arg)
        logp = d.gather(1, a[:, None])[:, 0] - log_total
        taken = ~stopped
        a = torch.where(taken, a, torch.full_like(a, abstain[r]))
        pred_none = a == abstain[r]
        if seq:
            length = torch.where(taken & pred_none, torch.full_like(length, r + 1), length)
            stopped = stopped | pred_none
        tg = targets[r].to(dev)
        gt_none = tg == null[r]
        oc = torch.where(gt_none, torch.where(pred_none, L.ABSTAIN_CORRECT_ABSTAIN, L.ABSTAIN_PREDICTED_AT_NULL),
                         torch.where(pred_none, L.ABSTAIN_UNNECESSARY_ABSTAIN, torch.where(a == tg, L.ABSTAIN_CORRECT, L.ABSTAIN_MISCLASSIFIED)))
        acts.append(a.to(torch.int32))
        logps.append(torch.where(taken, logp, torch.zeros_like(logp)))
        ents.append(torch.where(taken, H, torch.zeros_like(H)))
        takens.append(taken.to(torch.uint8))
        outcomes.append(oc)
    oc = torch.stack(outcomes, dim=1)  # [B, R]
    counted = 1 if reward.ranks == "first" else R
    if reward.kind == "simple":
        table = torch.tensor(reward.table, dtype=torch.float32, device=dev)
        rew = torch.zeros(B, device=dev)
        for r in range(counted):
            rew = rew + table[oc[:, r]]
    else:
        first_dev = _first_index(oc[:, :counted] != L.ABSTAIN_CORRECT)  # the first rank that is not a correct classification
        at = oc[:, :counted].gather(1, first_dev.clamp(max=counted - 1)[:, None])[:, 0]
        optimal = (first_dev == counted) | (at == L.ABSTAIN_CORRECT_ABSTAIN)
        rew = torch.where(optimal, reward.outcome[0], reward.outcome[1]).to(torch.float32)
    if counts is not None:
        for r in range(R):
            o = oc[:, r]
            per = [(o == L.ABSTAIN_CORRECT_ABSTAIN) | (o == L.ABSTAIN_UNNECESSARY_ABSTAIN), torch.ones_like(o, dtype=torch.bool),
                   o == L.ABSTAIN_CORRECT_ABSTAIN, o == L.ABSTAIN_UNNECESSARY_ABSTAIN, o == L.ABSTAIN_PREDICTED_AT_NULL, o == L.ABSTAIN_CORRECT,
                   o == L.ABSTAIN_MISCLASSIFIED]
            counts[L.ABSTAIN_CNT_STRIDE * r: L.ABSTAIN_CNT_STRIDE * r + 7] += torch.stack([m.sum() for m in per])
        counts[L.ABSTAIN_CNT_EPISODES] += B
        counts[L.ABSTAIN_CNT_LENGTH_SUM] += length.sum()
        counts[L.ABSTAIN_CNT_REWARD_FIX] += torch.round(rew * float(1 << L.ABSTAIN_REWARD_FIX_BITS)).to(torch.int64).sum()
    return Acted(torch.stack(acts, 1), torch.stack(logps, 1), torch.stack(ents, 1), torch.stack(takens, 1), length, rew)


# ------------------------------------------------------------------------------------------------------------------ advantages
def advantages(reward: torch.Tensor, value: torch.Tensor, length: torch.Tensor, mode, R: int, gamma: float = 0.99, gae_lambda: float = 0.95):
    """compute_gae_and_returns per whole episode, then the normalisation over all transitions of the rollout: (adv [B, R], ret [B, R],
    n_trans int32 [1]); multitask uses column 0.  Episodes are complete, so the reference's last_value never enters.  ONE launch."""
    mode = _mode_code(mode)
    if not abstention_on_device():
        return _advantages_torch(reward, value, length, mode, R, gamma, gae_lambda)
    B, dev = reward.shape[0], reward.device
    if not reward.is_cuda:
        raise L.LnxError("abstention: the HIP kernels need the rollout on the GPU (LNX_ABSTENTION=0 selects the torch composition)")
    reward, value = reward.detach().float().contiguous(), value.detach().float().contiguous()
    length = length.to(torch.int32).contiguous()
    if value.shape != (B,) or length.shape != (B,):
        raise L.LnxError(f"abstention: reward / value / length must all be [{B}]")
    adv, ret, n = torch.empty(B, R, device=dev), torch.empty(B, R, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    a = L.PpoAdvArgs()
    a.B, a.R, a.mode, a.gamma, a.gae_lambda = B, R, mode, gamma, gae_lambda
    a.reward, a.value, a.length, a.adv, a.ret, a.n_trans = (reward.data_ptr(), value.data_ptr(), length.data_ptr(), adv.data_ptr(), ret.data_ptr(),
                                                            n.data_ptr())
    L.check(L.lib().lnx_ppo_advantages(C.byref(a), _stream(dev)), "lnx_ppo_advantages")
    return adv, ret, n


def _advantages_torch(reward, value, length, mode, R, gamma, gae_lambda):
    B, dev = reward.shape[0], reward.device
    reward, V = reward.detach().float(), value.detach().float()
    Ln = length.to(torch.int64).clamp(1, R) if mode == L.ABSTAIN_SEQUENTIAL else torch.ones(B, dtype=torch.int64, device=dev)
    gamma_t, gl = torch.tensor(gamma, dtype=torch.float32, device=dev), torch.tensor(gamma, dtype=torch.float32, device=dev) * torch.tensor(
        gae_lambda, dtype=torch.float32, device=dev)
    cols, last = [None] * R, torch.zeros(B, device=dev)
    for t in range(R - 1, -1, -1):
        is_last = Ln == t + 1
        delta = torch.where(is_last, reward - V, gamma_t * V - V)
        last = torch.where(t < Ln, torch.where(is_last, delta, delta + gl * last), torch.zeros_like(V))
        cols[t] = last
    adv = torch.stack(cols, 1)
    mask = torch.arange(R, device=dev)[None, :] < Ln[:, None]
    ret = torch.where(mask, adv + V[:, None], torch.zeros_like(adv))
    n = mask.sum()
    mean = (adv.double() * mask).sum() / n
    sd = torch.sqrt((((adv.double() - mean) ** 2) * mask).sum() / n)
    adv = torch.where(mask, (adv - mean.float()) / (sd.float() + 1e-8), torch.zeros_like(adv))
    return adv, ret, n.to(torch.int32).reshape(1)


# ------------------------------------------------------------------------------------------------------------------ loss
def loss_forward(logits, value, actions, taken, logp_old, adv, ret, mode, eps, vf, ent):
    """lnx_ppo_loss_fwd on plain tensors: (args, out).  `args` is the filled lnx_ppo_loss_args for `loss_backward`; it holds addresses,
    the tensors behind them are kept alive in args._keep."""
    xs = _prep_logits(logits)
    B, R, dev = xs[0].shape[0], len(xs), xs[0].device
    a = L.PpoLossArgs()
    a.dtype, a.B, a.R, a.mode = (L.BF16 if xs[0].dtype == torch.bfloat16 else L.F32), B, R, _mode_code(mode)
    a.clip_eps, a.vf_coef, a.ent_coef = eps, vf, ent
    keep = [actions.to(torch.int32).contiguous(), taken.to(torch.uint8).contiguous(), logp_old.detach().float().contiguous(),
            adv.detach().float().contiguous(), ret.detach().float().contiguous(), value.detach().float().contiguous()]
    for t in keep[:5]:
        if t.shape != (B, R) or t.device != dev:
            raise L.LnxError(f"ppo_loss: actions / taken / logp_old / adv / ret must be [{B}, {R}] on {dev}")
    if keep[5].shape != (B,):
        raise L.LnxError(f"ppo_loss: value must be [{B}], got {tuple(keep[5].shape)}")
    a.actions, a.taken, a.logp_old, a.adv, a.ret, a.value = [t.data_ptr() for t in keep]
    ws = torch.empty(R * L.PPO_WS_ROWS * B, device=dev)
    out = torch.empty(L.PPO_OUT_FLOATS, device=dev)
    a.ws, a.out = ws.data_ptr(), out.data_ptr()
    _fill_ranks(a.rank, xs)
    L.check(L.lib().lnx_ppo_loss_fwd(C.byref(a), _stream(dev)), "lnx_ppo_loss_fwd")
    a._keep, a._xs = keep + [ws, out], xs
    return a, out


def loss_backward(a, go: torch.Tensor, dlogits: Sequence[Optional[torch.Tensor]], dvalue: Optional[torch.Tensor]) -> None:
    """lnx_ppo_loss_bwd into the caller's buffers: dlogits[r] fp32 [B, >= C_r] row views or None, dvalue fp32 [B] or None.  Columns
    >= C_r and the rows of untaken ranks are left as they are."""
    go = go.detach().float().reshape(1).contiguous()
    a.dvalue = None if dvalue is None else dvalue.data_ptr()
    for r, d in enumerate(dlogits):
        a.rank[r].dlogits, a.rank[r].ldd = (None, 0) if d is None else (d.data_ptr(), d.stride(0) if d.shape[0] > 1 else d.shape[1])
    L.check(L.lib().lnx_ppo_loss_bwd(C.byref(a), C.c_void_p(go.data_ptr()), _stream(go.device)), "lnx_ppo_loss_bwd")


class _PpoLossFn(torch.autograd.Function):
    """lnx_ppo_loss_fwd (2 launches) / lnx_ppo_loss_bwd (1 launch).  Outputs: the total loss and the detached out[] vector."""

    @staticmethod
    def forward(ctx, meta, value, *logits):
        ctx.args, out = loss_forward(logits, value, *meta)
        ctx.needs = (ctx.needs_input_grad[1], ctx.needs_input_grad[2:])
        ctx.mark_non_differentiable(out)
        return out[L.PPO_OUT_TOTAL].clone(), out

    @staticmethod
    def backward(ctx, go, _gout):
        a, xs = ctx.args, ctx.args._xs
        B, dev = xs[0].shape[0], xs[0].device
        need_v, need_x = ctx.needs
        # zeros: the rows of untaken ranks are not written and get no gradient
        dl = [torch.zeros(B, x.shape[1], device=dev) if n else None for x, n in zip(xs, need_x)]
        dv = torch.empty(B, device=dev) if need_v else None
        if dv is not None or any(d is not None for d in dl):
            loss_backward(a, go, dl, dv)
        return (None, dv) + tuple(None if d is None else d.to(x.dtype) for d, x in zip(dl, xs))


def ppo_loss(logits: Sequence[torch.Tensor], value: torch.Tensor, actions, taken, logp_old, adv, ret, mode="sequential", clip_epsilon: float = 0.2,
             vf_coef: float = 0.5, ent_coef: float = 0.01):
    """The clipped-surrogate loss of a minibatch of B samples with all their steps, each step evaluated at its own rank (finding F-d).
    Returns (total, stats): total carries the gradient to the logits and the value; stats is a detached dict of device scalars
    (policy_loss, value_loss, entropy_loss, total_loss, n, ratio_mean, clip_frac)."""
    mode = _mode_code(mode)
    if abstention_on_device():
        if not logits[0].is_cuda:
            raise L.LnxError("abstention: the HIP kernels need the logits on the GPU (LNX_ABSTENTION=0 selects the torch composition)")
        total, out = _PpoLossFn.apply((actions, taken, logp_old, adv, ret, mode, float(clip_epsilon), float(vf_coef), float(ent_coef)), value, *logits)
    else:
        total, out = _ppo_loss_torch(logits, value, actions, taken, logp_old, adv, ret, mode, clip_epsilon, vf_coef, ent_coef)
    names = ("policy_loss", "value_loss", "entropy_loss", "total_loss", "n", "ratio_mean", "clip_frac")
    return total, {k: out[i] for i, k in enumerate(names)}


def _ppo_loss_torch(logits, value, actions, taken, logp_old, adv, ret, mode, eps, vf, ent):
    R = len(logits)
    seq = mode == L.ABSTAIN_SEQUENTIAL
    lps, Hs = [], []
    for r in range(R):
        ls = torch.log_softmax(logits[r].float(), dim=1)
        p = ls.exp()
        lps.append(ls.gather(1, actions[:, r].long()[:, None])[:, 0])
        Hs.append(-torch.where(p > 0, p * ls, torch.zeros_like(p)).sum(dim=1))
    dlp, H = torch.stack(lps, 1) - logp_old.detach().float(), torch.stack(Hs, 1)  # (the differences are summed, not the sums subtracted)
    V = value.float()
    if seq:
        mask = taken.bool()
        A, rt, Vt = adv.float(), ret.float(), V[:, None].expand(-1, R)
    else:
        mask = torch.ones(dlp.shape[0], 1, dtype=torch.bool, device=dlp.device)
        dlp, H = dlp.sum(1, keepdim=True), H.sum(1, keepdim=True)
        A, rt, Vt = adv[:, :1].float(), ret[:, :1].float(), V[:, None]
    n = mask.sum()
    zero = torch.zeros((), device=dlp.device)
    ratio = torch.exp(torch.where(mask, dlp, zero))
    surr = torch.min(ratio * A, torch.clamp(ratio, 1.0 - eps, 1.0 + eps) * A)

    def mean(v):
        return torch.where(mask, v, zero).sum() / n

    policy, val, entl = -mean(surr), mean((Vt - rt) ** 2), -mean(H)
    total = policy + vf * val + ent * entl
    clipped = ((ratio < 1.0 - eps) | (ratio > 1.0 + eps)).float()
    out = torch.stack([policy, val, entl, total, n.float(), mean(ratio), mean(clipped), zero]).detach()
    return total, out


# ------------------------------------------------------------------------------------------------------------------ policy
def _rank_number(task_key: str) -> int:
    return int(task_key.split("_L")[-1])


class AbstentionPolicy(nn.Module):
    """The model's heads as the policy and one linear value head on its features.  One `model._run` per call gives features and logits
    together (the reference's wrapper runs the model twice per decision and needs a `.backbone` mFormerV1 does not have); the gradients
    of both flow back through the plan's single backward.

    rank_order: task keys in DECISION order; default coarsest first (descending `_L<n>`), because an abstention ends a sequential
    episode (the reference walks taxonomy_tree.task_keys as they come, finding F-c).  abstain_index / null_index: an int for every
    rank or one per rank, in decision order: the class of each head that means "abstain" (finding F-b), and the target that is the
    ground truth None."""

    def __init__(self, model, mode: str = "sequential", rank_order: Optional[Sequence[str]] = None, abstain_index=0, null_index=0):
        super().__init__()
        if mode not in MODES:
            raise ValueError(f"AbstentionPolicy: mode={mode!r} (multitask or sequential)")
        self.model, self.mode = model, mode
        tasks = list(model.task_keys)
        self.rank_order = list(rank_order) if rank_order is not None else sorted(tasks, key=_rank_number, reverse=True)
        unknown = [t for t in self.rank_order if t not in tasks]
        if unknown or not 1 <= len(self.rank_order) <= L.METRICS_MAX_TASKS or len(set(self.rank_order)) != len(self.rank_order):
            raise ValueError(f"AbstentionPolicy: rank_order={self.rank_order} must name 1..{L.METRICS_MAX_TASKS} distinct tasks of {tasks}")
        R = len(self.rank_order)
        self.num_classes = [model.head[t].effective_linear.out_features for t in self.rank_order]
        self.abstain_index, self.null_index = _per_rank(abstain_index, R, "abstain_index"), _per_rank(null_index, R, "null_index")
        for t, c, ai, ni in zip(self.rank_order, self.num_classes, self.abstain_index, self.null_index):
            if not (0 <= ai < c and 0 <= ni < c):
                raise ValueError(f"AbstentionPolicy: abstain_index={ai} / null_index={ni} of {t} outside [0, {c})")
        self.value_head = nn.Linear(model.head[self.rank_order[0]].effective_linear.in_features, 1)

    def forward(self, images: torch.Tensor, meta: Optional[torch.Tensor] = None):
        """(logits per rank in decision order, value [B]) from one pass of the plan.  The value head is a torch matmul: the library's
        skinny GEMM takes bf16 operands only and `heads.hip_linear` keeps fp32, so an N = 1 product would go to the 128x128 tile kernel."""
        st, feats, views = self.model._run(images, meta)
        by_task = dict(zip(st["tasks"], views))
        value = torch.nn.functional.linear(feats.float(), self.value_head.weight, self.value_head.bias)[:, 0]
        return [by_task[t] for t in self.rank_order], value

    def targets_in_order(self, targets: Dict[str, torch.Tensor]) -> List[torch.Tensor]:
        """{task: int [B] or soft [B, C]} -> int64 [B] per rank in decision order; a soft target is taken at its arg-max
        (rl_env/problem_provider.py:154-164)"""
        out = []
        for t in self.rank_order:
            v = targets[t]
            out.append((v.argmax(dim=1) if v.dim() == 2 else v).to(torch.int64))
        return out


class Rollout(NamedTuple):
    """a device-side batch of transitions: what `ppo_update` needs to evaluate the same decisions again"""
    images: torch.Tensor
    meta: Optional[torch.Tensor]
    acted: Acted
    value: torch.Tensor    # fp32 [B], detached
    adv: torch.Tensor      # fp32 [B, R], normalised over the rollout
    ret: torch.Tensor      # fp32 [B, R]
    n_trans: torch.Tensor  # int32 [1]
    u: Optional[torch.Tensor]


def rollout(policy: AbstentionPolicy, images: torch.Tensor, meta: Optional[torch.Tensor], targets: Dict[str, torch.Tensor],
            reward: Optional[AbstentionReward] = None, generator: Optional[torch.Generator] = None, greedy: bool = False, gamma: float = 0.99,
            gae_lambda: float = 0.95, counts: Optional[torch.Tensor] = None, u: Optional[torch.Tensor] = None) -> Rollout:
    """One episode per image in either mode from ONE no_grad forward, then lnx_abstain_act and lnx_ppo_advantages; nothing is read back.
    The uniforms are torch's (generator; or given as u [B, R])."""
    with torch.no_grad():
        logits, value = policy(images, meta)
        B, R = images.shape[0], len(logits)
        if u is None and not greedy:
            u = torch.rand(B, R, device=images.device, generator=generator)
        acted = act(logits, [t.to(images.device) for t in policy.targets_in_order(targets)], u, policy.mode, greedy, reward, policy.abstain_index,
                    policy.null_index, counts)
        adv, ret, n = advantages(acted.reward, value, acted.length, policy.mode, R, gamma, gae_lambda)
    return Rollout(images, meta, acted, value.detach(), adv, ret, n, u)


def ppo_update(policy: AbstentionPolicy, optimizer, batch: Rollout, ppo_epochs: int = 4, minibatch: int = 64, clip_epsilon: float = 0.2,
               vf_coef: float = 0.5, ent_coef: float = 0.01, max_grad_norm: float = 0.5, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
    """ppo_update of rl_train_abstention.py:57-131 on a `Rollout`.  A minibatch is a set of SAMPLES with all their steps (finding F-d):
    one forward, the fused loss (3 launches), one backward, the clip and the step.  The clip is the optimizer's own where it has one
    (FusedAdamW / FusedAdEMAMix / FusedSGD / FusedMuon / FusedMultiOptimizer: `max_grad_norm`, set for the duration of the update),
    clip_grad_norm_ otherwise.  Returns the last minibatch's loss components as device scalars (what the reference logs)."""
    from .optim import _Clipped

    B = batch.images.shape[0]
    dev = batch.images.device
    own_clip = isinstance(optimizer, _Clipped)
    params = [p for p in policy.parameters() if p.requires_grad]
    was_training = policy.training
    before = optimizer.max_grad_norm if own_clip else None
    if own_clip:
        optimizer.max_grad_norm = float(max_grad_norm) if max_grad_norm and max_grad_norm > 0 else None
    policy.train()
    stats: Dict[str, torch.Tensor] = {}
    try:
        for _ in range(int(ppo_epochs)):
            perm = torch.randperm(B, device=dev, generator=generator) if minibatch < B else None
            for start in range(0, B, minibatch):
                if perm is None:
                    sel = lambda t: t  # noqa: E731  (the whole rollout, in order)
                else:
                    idx = perm[start: start + minibatch]
                    sel = lambda t, idx=idx: t.index_select(0, idx)  # noqa: E731
                ac = batch.acted
                logits, value = policy(sel(batch.images), None if batch.meta is None else sel(batch.meta))
                total, stats = ppo_loss(logits, value, sel(ac.actions), sel(ac.taken), sel(ac.logp), sel(batch.adv), sel(batch.ret), policy.mode,
                                        clip_epsilon, vf_coef, ent_coef)
                optimizer.zero_grad()
                total.backward()
                if not own_clip and max_grad_norm and max_grad_norm > 0:
                    torch.nn.utils.clip_grad_norm_(params, max_norm=max_grad_norm)
                optimizer.step()
    finally:
        if own_clip:
            optimizer.max_grad_norm = before
        policy.train(was_training)
    return stats


def results_from_counts(counts, rank_order: Sequence[str], median_reward=None) -> Dict[str, float]:
    """the result keys of the reference's evaluate_policy from a counter table on the host (a list or tensor of LNX_ABSTAIN_COUNTS ints)"""
    c = [int(v) for v in (counts.tolist() if isinstance(counts, torch.Tensor) else counts)]
    n = c[L.ABSTAIN_CNT_EPISODES]
    res = {"mean_reward": c[L.ABSTAIN_CNT_REWARD_FIX] / float(1 << L.ABSTAIN_REWARD_FIX_BITS) / n if n else 0,
           "median_reward": (median_reward if median_reward is not None else 0) if n else 0,
           "mean_length": c[L.ABSTAIN_CNT_LENGTH_SUM] / n if n else 0}
    for r, name in enumerate(rank_order):
        k = dict(zip(COUNTERS, c[L.ABSTAIN_CNT_STRIDE * r: L.ABSTAIN_CNT_STRIDE * r + 7]))
        total, abst = k["total_decisions"], k["abstained"]
        should = k["correct_abstain"] + k["missed_abstain"]
        classified = k["correct_classify_non_abstain"] + k["misclassify_non_abstain"]
        res[f"abst_rate/{name}"] = abst / total if total > 0 else 0
        res[f"corr_abst_rate/{name}"] = k["correct_abstain"] / abst if abst > 0 else 0
        res[f"unnec_abst_rate/{name}"] = k["unnecessary_abstain"] / abst if abst > 0 else 0
        res[f"recall_abst/{name}"] = k["correct_abstain"] / should if should > 0 else 0
        res[f"acc_on_non_abst/{name}"] = k["correct_classify_non_abstain"] / classified if classified > 0 else 0
        res[f"missed_abst_count/{name}"] = k["missed_abstain"]
    return res


def evaluate_policy(policy: AbstentionPolicy, loader, reward: Optional[AbstentionReward] = None, return_counts: bool = False):
    """evaluate_policy of rl_train_abstention.py:133-207 over a loader of (images, meta, targets) batches: greedy episodes, every
    counter added on the device (lnx_abstain_act with a counter table), ONE read-back at the end.  The loader's images are on the
    device already.  Returns the reference's result keys; with return_counts also the raw counter list."""
    was_training = policy.training
    policy.eval()
    counts, rewards = None, []
    try:
        for images, meta, targets in loader:
            if counts is None:
                counts = new_counts(images.device)
            rewards.append(rollout(policy, images, meta, targets, reward=reward, greedy=True, counts=counts).acted.reward)
    finally:
        policy.train(was_training)
    if counts is None:
        res = results_from_counts([0] * L.ABSTAIN_COUNTS, policy.rank_order)
        return (res, [0] * L.ABSTAIN_COUNTS) if return_counts else res
    # one copy: the counters and the bit pattern of the median reward (np.median's: the mean of the two middle values)
    med = torch.quantile(torch.cat(rewards).double(), 0.5).reshape(1).view(torch.int64)
    host = torch.cat([counts, med]).cpu()
    res = results_from_counts(host[:-1], policy.rank_order, float(host[-1:].view(torch.float64)))
    return (res, host[:-1].tolist()) if return_counts else res
