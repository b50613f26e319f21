"""CPU restatement of lnx_hier_refine_fwd / lnx_hier_refine_bwd (include/lnx.h) in fp64: the forward as the formula, the backward
written out by hand (no autograd).  Levels come finest first.  `storage` (None, torch.float32 or torch.bfloat16) rounds each level's
finished row -- the refined logits in the forward, G in the backward -- to that type before the next level reads it, which is what
the kernels do with their tensors; None keeps everything in fp64."""
import torch

SOFT, HARD, GUMBEL = 0, 1, 2
EPS = 1e-10


def _store(x, storage):
    return x if storage is None else x.to(storage).double()


def routing_probs(R, mode, temperature=1.0, noise=None):
    """The reference's _compute_routing_probabilities (conditional_classifier_head.py:142-160) on fp64 rows."""
    R = R.double()
    if mode == HARD:
        return torch.zeros_like(R).scatter_(1, R.argmax(dim=1, keepdim=True), 1.0)
    if mode == GUMBEL:
        R = R + noise.double()
    return torch.softmax(R / temperature, dim=1)


def _gather(prob, parent):
    """prior[:, c] = prob[:, parent[c]], 0 where parent[c] < 0"""
    parent = parent.long()
    prior = prob[:, parent.clamp(min=0)]
    return torch.where(parent.ge(0).unsqueeze(0), prior, torch.zeros_like(prior))


def forward(bases, parents, modes=None, temps=None, noises=None, storage=None):
    """bases: per level [B, C]; parents: per level an integer [C] table (-1 = none) or None (pass-through; the last entry is not
    read).  Returns the refined rows per level in fp64 (holding `storage`-rounded values)."""
    T = len(bases)
    modes = modes or [SOFT] * T
    temps = temps or [1.0] * T
    noises = noises or [None] * T
    outs = [None] * T
    for t in range(T - 1, -1, -1):
        x = bases[t].double()
        if t < T - 1 and parents[t] is not None:
            prob = routing_probs(outs[t + 1], modes[t], temps[t], noises[t])
            x = x + torch.log(_gather(prob, parents[t]) + EPS)
        outs[t] = _store(x, storage)
    return outs


def backward(outs, douts, parents, modes=None, temps=None, noises=None, storage=None):
    """outs: what forward returned; douts: per level [B, C] or None (= zeros).  Returns the gradient of every level's base logits:
    G_t = dout_t + (what level t - 1 sends up), finest level first."""
    T = len(outs)
    modes = modes or [SOFT] * T
    temps = temps or [1.0] * T
    noises = noises or [None] * T
    G = [None] * T
    for t in range(T):
        g = torch.zeros_like(outs[t]) if douts[t] is None else douts[t].double().clone()
        if t > 0 and parents[t - 1] is not None and modes[t - 1] != HARD:
            parent = parents[t - 1].long()
            has = parent.ge(0)
            S = torch.zeros_like(outs[t]).index_add_(1, parent[has], G[t - 1][:, has])
            prob = routing_probs(outs[t], modes[t - 1], temps[t - 1], noises[t - 1])
            dprob = S / (prob + EPS)
            g = g + prob * (dprob - (prob * dprob).sum(1, keepdim=True)) / temps[t - 1]
        G[t] = _store(g, storage)
    return G


def random_parents(n_child, n_parent, gen, orphan_every=0, barren=(), crowd=None):
    """A parent table: child c -> a seeded parent, never one of `barren` (parents left without children); every `orphan_every`-th
    child gets -1; `crowd` = (parent, count): the first `count` children all go to that parent."""
    allowed = torch.tensor([j for j in range(n_parent) if j not in set(barren)] or [0])
    par = allowed[torch.randint(0, allowed.numel(), (n_child,), generator=gen)]
    if crowd is not None:
        par[: crowd[1]] = crowd[0]
    if orphan_every:
        par[orphan_every - 1 :: orphan_every] = -1
    return par.to(torch.int32)
