"""fp64 restatement of the abstention phase (include/lnx.h: lnx_abstain_act, lnx_ppo_advantages, lnx_ppo_loss_fwd / _bwd), written
from the definitions and independent of linnaeus_amd/rl.py: torch.distributions.Categorical for log-probabilities and entropies, a
sequential inverse CDF, the reference's reward walks and GAE recursion as plain Python, the loss through autograd."""
import numpy as np
import torch

SIMPLE_DEFAULT = (1.0, 0.5, -1.0, -0.5, -1.0)  # correct, correct_abstain, misclassified, unnecessary_abstain, predicted_at_null
OUTCOME_DEFAULT = (1.0, -1.0)
CORRECT, CORRECT_ABSTAIN, MISCLASSIFIED, UNNECESSARY_ABSTAIN, PREDICTED_AT_NULL = range(5)
COUNTERS = ("abstained", "total_decisions", "correct_abstain", "unnecessary_abstain", "missed_abstain", "correct_classify_non_abstain",
            "misclassify_non_abstain")
CNT_STRIDE, CNT_EPISODES, CNT_LENGTH_SUM, CNT_REWARD_FIX, N_COUNTS, FIX_BITS = 8, 64, 65, 66, 72, 20


def outcome_of(pred, gt):
    """the table of the issue: labels are ints or None"""
    if gt is None:
        return CORRECT_ABSTAIN if pred is None else PREDICTED_AT_NULL
    if pred is None:
        return UNNECESSARY_ABSTAIN
    return CORRECT if pred == gt else MISCLASSIFIED


def simple_reward(preds, gts, table=SIMPLE_DEFAULT):
    """SimpleAbstentionReward.compute_reward over the given ranks (Python floats, in rank order)"""
    total = 0.0
    for p, g in zip(preds, gts):
        total += table[outcome_of(p, g)]
    return total


def outcome_reward(preds, gts, values=OUTCOME_DEFAULT):
    """EpisodeOutcomeReward.compute_reward: optimal up to and including the first correct abstention, or throughout"""
    for p, g in zip(preds, gts):
        o = outcome_of(p, g)
        if o == CORRECT:
            continue
        return values[0] if o == CORRECT_ABSTAIN else values[1]
    return values[0]


def episode_reward(preds, gts, kind="simple", ranks="all", table=SIMPLE_DEFAULT, values=OUTCOME_DEFAULT):
    """ranks="all": the list form {"k": [p0, p1, ...]}; ranks="first": what {rank: [label]} gives in the reference (finding F-a)"""
    if ranks == "first":
        preds, gts = preds[:1], gts[:1]
    return simple_reward(preds, gts, table) if kind == "simple" else outcome_reward(preds, gts, values)


def row_reference(z):
    """z: [B, C] float64 -> (greedy [B], entropy [B], cdf [B, C]): torch's Categorical and a running sum in class order"""
    z = z.double()
    dist = torch.distributions.Categorical(logits=z)
    mx = z.max(dim=1, keepdim=True).values
    greedy = torch.where(z == mx, torch.arange(z.shape[1]).expand_as(z), torch.full(z.shape, z.shape[1], dtype=torch.int64)).min(dim=1).values
    e = torch.exp(z - mx)
    cdf = torch.cumsum(e, dim=1)
    return greedy, dist.entropy(), cdf / cdf[:, -1:]


def inverse_cdf(cdf, u, greedy):
    """the smallest j with cdf[j] > u (the greedy class if none), and the distance of u to the nearer boundary of that class"""
    B, C = cdf.shape
    hit = cdf > u.double()[:, None]
    j = torch.where(hit, torch.arange(C).expand_as(hit), torch.full(hit.shape, C, dtype=torch.int64)).min(dim=1).values
    a = torch.where(j < C, j, greedy)
    hi = cdf.gather(1, a[:, None])[:, 0]
    lo = torch.where(a > 0, cdf.gather(1, (a - 1).clamp(min=0)[:, None])[:, 0], torch.zeros(B, dtype=torch.float64))
    return a, torch.minimum(u.double() - lo, hi - u.double())


def rollout_ref(logits, targets, u, mode, greedy=False, kind="simple", ranks="all", table=SIMPLE_DEFAULT, values=OUTCOME_DEFAULT, abstain=None,
                null=None, forced_actions=None):
    """logits / targets per rank in decision order (CPU; bf16 inputs are taken at their rounded values).  forced_actions [B, R]: take
    these at every taken rank in place of the restatement's own draw (the kernel's action, so that everything downstream is compared
    at the same decision).  Returns a dict of CPU tensors and a Python list of counters."""
    R, B = len(logits), logits[0].shape[0]
    abstain = [0] * R if abstain is None else list(abstain)
    null = [0] * R if null is None else list(null)
    seq = mode == "sequential"
    own = torch.zeros(B, R, dtype=torch.int64)
    margin = torch.full((B, R), float("inf"), dtype=torch.float64)
    greedy_cls = torch.zeros(B, R, dtype=torch.int64)
    actions = torch.zeros(B, R, dtype=torch.int64)
    logp = torch.zeros(B, R, dtype=torch.float64)
    ent = torch.zeros(B, R, dtype=torch.float64)
    taken = torch.zeros(B, R, dtype=torch.uint8)
    stopped = torch.zeros(B, dtype=torch.bool)
    for r in range(R):
        z = logits[r].double()
        g, H, cdf = row_reference(z)
        greedy_cls[:, r] = g
        if greedy:
            a = g
        else:
            a, m = inverse_cdf(cdf, u[:, r], g)
            margin[:, r] = m
        own[:, r] = a
        if forced_actions is not None:
            a = forced_actions[:, r].to(torch.int64)
        lp = torch.distributions.Categorical(logits=z).log_prob(a.clamp(0, z.shape[1] - 1))
        tk = ~stopped
        actions[:, r] = torch.where(tk, a, torch.full_like(a, abstain[r]))
        logp[:, r] = torch.where(tk, lp, torch.zeros_like(lp))
        ent[:, r] = torch.where(tk, H, torch.zeros_like(H))
        taken[:, r] = tk.to(torch.uint8)
        if seq:
            stopped = stopped | (actions[:, r] == abstain[r])
    length = taken.sum(dim=1).to(torch.int32) if seq else torch.ones(B, dtype=torch.int32)
    counts = [0] * N_COUNTS
    reward = torch.zeros(B, dtype=torch.float64)
    acts, tgs = actions.tolist(), [t.tolist() for t in targets]
    for b in range(B):
        preds = [None if (not taken[b, r] or acts[b][r] == abstain[r]) else acts[b][r] for r in range(R)]
        gts = [None if tgs[r][b] == null[r] else tgs[r][b] for r in range(R)]
        rew = episode_reward(preds, gts, kind, ranks, table, values)
        reward[b] = rew
        for r in range(R):
            c = dict.fromkeys(COUNTERS, 0)
            c["total_decisions"] += 1  # the counting block of evaluate_policy
            if preds[r] is None:
                c["abstained"] += 1
                c["correct_abstain" if gts[r] is None else "unnecessary_abstain"] += 1
            elif gts[r] is None:
                c["missed_abstain"] += 1
            else:
                c["correct_classify_non_abstain" if preds[r] == gts[r] else "misclassify_non_abstain"] += 1
            for i, name in enumerate(COUNTERS):
                counts[CNT_STRIDE * r + i] += c[name]
        counts[CNT_EPISODES] += 1
        counts[CNT_LENGTH_SUM] += int(length[b])
        counts[CNT_REWARD_FIX] += int(round(rew * (1 << FIX_BITS)))
    return {"actions": actions, "own_actions": own, "margin": margin, "greedy": greedy_cls, "logp": logp, "entropy": ent, "taken": taken,
            "length": length, "reward": reward, "counts": counts}


def gae_and_returns(rewards, values, dones, last_value, gamma, gae_lambda):
    """the recursion of compute_gae_and_returns (rl_train_abstention.py:38-55) on float64 arrays"""
    n = len(rewards)
    adv = np.zeros(n, dtype=np.float64)
    last = 0.0
    for t in reversed(range(n)):
        non_terminal = 1.0 - dones[t]
        next_value = last_value if t == n - 1 else values[t + 1]
        delta = rewards[t] + gamma * next_value * non_terminal - values[t]
        adv[t] = last = delta + gamma * gae_lambda * non_terminal * last
    return adv, adv + np.asarray(values, dtype=np.float64)


def advantages_ref(reward, value, length, mode, R, gamma=0.99, gae_lambda=0.95):
    """per episode the recursion above (the episode's last step is done: last_value is multiplied by 1 - done = 0 and never enters), then
    (adv - mean) / (std + 1e-8) over all transitions with the population std: (adv [B, R], ret [B, R], N) in float64"""
    B = len(reward)
    adv, ret = np.zeros((B, R)), np.zeros((B, R))
    for b in range(B):
        L = int(length[b]) if mode == "sequential" else 1
        rewards = np.zeros(L)
        rewards[-1] = float(reward[b])
        dones = np.zeros(L)
        dones[-1] = 1.0
        a, r = gae_and_returns(rewards, np.full(L, float(value[b])), dones, 0.0, gamma, gae_lambda)
        adv[b, :L], ret[b, :L] = a, r
    steps = np.asarray(length).astype(np.int64) if mode == "sequential" else np.ones(B, dtype=np.int64)
    mask = np.arange(R)[None, :] < steps[:, None]
    flat = adv[mask]
    adv = np.where(mask, (adv - flat.mean()) / (flat.std() + 1e-8), 0.0)
    return torch.from_numpy(adv), torch.from_numpy(ret), int(mask.sum())


def ppo_loss_ref(logits, value, actions, taken, logp_old, adv, ret, mode, eps=0.2, vf=0.5, ent=0.01):
    """the loss of ppo_update (rl_train_abstention.py:109-116) in float64 through autograd, each decision at its own rank.
    Returns (dict of floats, [dlogits per rank], dvalue)."""
    R, B = len(logits), logits[0].shape[0]
    zs = [x.detach().double().clone().requires_grad_(True) for x in logits]
    V = value.detach().double().clone().requires_grad_(True)
    lps, Hs = [], []
    for r in range(R):
        dist = torch.distributions.Categorical(logits=zs[r])
        lps.append(dist.log_prob(actions[:, r].to(torch.int64)))
        Hs.append(dist.entropy())
    lp, H, lo = torch.stack(lps, 1), torch.stack(Hs, 1), logp_old.double()
    if mode == "sequential":
        idx = taken.bool()
        lp, H, lo, A, rt, Vt = lp[idx], H[idx], lo[idx], adv.double()[idx], ret.double()[idx], V[:, None].expand(B, R)[idx]
    else:
        lp, H, lo, A, rt, Vt = lp.sum(1), H.sum(1), lo.sum(1), adv.double()[:, 0], ret.double()[:, 0], V
    ratio = torch.exp(lp - lo)
    policy = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - eps, 1.0 + eps) * A).mean()
    val = torch.nn.functional.mse_loss(Vt, rt)
    entl = -H.mean()
    total = policy + vf * val + ent * entl
    total.backward()
    out = {"policy_loss": policy.item(), "value_loss": val.item(), "entropy_loss": entl.item(), "total_loss": total.item(), "n": float(lp.numel()),
           "ratio_mean": ratio.mean().item(), "clip_frac": float(((ratio < 1.0 - eps) | (ratio > 1.0 + eps)).double().mean())}
    return out, [z.grad if z.grad is not None else torch.zeros_like(z) for z in zs], V.grad
