"""Plain-torch CPU restatement of one whole Muon step (linnaeus/optimizers/muon.py:126-190) on
oracle.mformer_oracle.newton_schulz5 (the reference's round-everything bf16 iteration), or with `exact=True` on
newton_schulz5_exact (the same iteration in fp64).  tests/golden/muon_fused.npz pins it to the reference's own Muon bit
for bit on the CPU (tests/test_muon_fused_host.py); the GPU tests of FusedMuon then use it as their reference at any shape.

A group is a dict with lr, weight_decay, momentum, nesterov, ns_steps.  Nothing is modified in place.
"""
import torch

from oracle import mformer_oracle as O


def scaling(shape) -> float:
    """max(1, rows / cols)^(1/2) with cols = in * kh * kw for a 4-D parameter (muon.py:177-185)"""
    rows, cols = shape[0], 1
    for s in shape[1:]:
        cols *= s
    return max(1, rows / cols) ** 0.5


def momentum_update(g, buf, group):
    """(new momentum buffer, the gradient the orthogonalisation sees): muon.py:159-167"""
    buf = (torch.zeros_like(g) if buf is None else buf.clone()).lerp_(g, 1 - group["momentum"])
    return buf, (g.clone().lerp_(buf, group["momentum"]) if group["nesterov"] else buf.clone())


def orthogonalised(u, group, exact=False):
    """the update direction O of a momentum gradient u, in the parameter's shape (fp32, or fp64 when exact)"""
    u2 = u.view(u.size(0), -1) if u.ndim == 4 else u
    o = O.newton_schulz5_exact(u2, steps=group["ns_steps"]) if exact else O.newton_schulz5(u2, steps=group["ns_steps"]).float()
    return o.reshape(u.shape)


def step(p, g, buf, group, exact=False):
    """one step of one parameter: (new p, new buf, O); g None: skipped (p, buf, None).  With exact=True O is the fp64 iteration's
    and p is updated in fp64 from it (returned as fp64)."""
    if g is None:
        return p, buf, None
    lr = group["lr"]
    buf, u = momentum_update(g, buf, group)
    o = orthogonalised(u, group, exact)
    if exact:
        q = p.double() * (1 - lr * group["weight_decay"]) - lr * scaling(p.shape) * o
        return q, buf, o
    q = p.clone()
    if group["weight_decay"] != 0:
        q.mul_(1 - lr * group["weight_decay"])
    q.add_(o.bfloat16(), alpha=-lr * scaling(p.shape))
    return q, buf, o


def recover_update(p_old, p_new, group):
    """U = (p (1 - lr wd) - p_new) / (lr s): the orthogonalised update a step applied, recovered from the parameters"""
    lr = group["lr"]
    return (p_old * (1 - lr * group["weight_decay"]) - p_new) / (lr * scaling(p_old.shape))
