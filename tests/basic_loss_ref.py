"""CPU restatement, in plain torch and float64, of the three criteria of linnaeus_amd.loss that follow the reference's
loss/basic_loss.py, written from the row arithmetic of include/lnx.h (lnx_softce):

    loss[b]       = cw[b] * (lse[b] * sum_c S[b, c] - sum_c S[b, c] x[b, c])
    dlogits[b, :] = go[b] * cw[b] * (exp(x[b, :] - lse[b]) * sum_c S[b, c] - S[b, :])

    "ce"  S = one-hot(class)                                      cw = weight[class]
    "ls"  S = 1 - eps at the class, eps / (C - 1) elsewhere        cw = weight[class]
    "st"  S = target[b, :] (sum S is summed, not assumed to be 1)  cw = sum_c target[b, c] * weight[c]

class = target[b], or the first maximum of a [B, C] target ("ce" / "ls").  A row whose class is ignore_index has loss 0 and gradient 0.
A class outside [0, C), and an "st" row whose sum is not finite, has a NaN loss and a zero gradient row.  Nothing here is taken from the
code under test: tests/test_basic_loss.py holds this file against the reference's recorded numbers, the GPU tests hold the kernels
against this file."""
import torch


def basic_ref(kind, x, target, weight=None, ignore_index=None, smoothing=0.0, go=None):
    """(loss [B], dlogits [B, C]) in float64; `go` [B] is the upstream gradient of the per-sample losses (ones when None)"""
    x = torch.as_tensor(x).double()
    B, C = x.shape
    target = torch.as_tensor(target)
    go = torch.ones(B, dtype=torch.float64) if go is None else torch.as_tensor(go).double()
    w = None if weight is None else torch.as_tensor(weight).double()
    lse = torch.logsumexp(x, 1)
    if kind == "st":
        assert target.dim() == 2 and ignore_index is None
        S = target.double()
        bad = ~torch.isfinite(S.sum(1))
        ignored = torch.zeros(B, dtype=torch.bool)
        cw = torch.ones(B, dtype=torch.float64) if w is None else (S * w[None, :]).sum(1)
    else:
        cls = target.argmax(1) if target.dim() == 2 else target.long()
        bad = (cls < 0) | (cls >= C)
        safe = torch.where(bad, torch.zeros_like(cls), cls)
        if kind == "ce":
            S = torch.zeros(B, C, dtype=torch.float64)
            S[torch.arange(B), safe] = 1.0
        elif kind == "ls":
            assert C > 1
            S = torch.full((B, C), float(smoothing) / (C - 1), dtype=torch.float64)
            S[torch.arange(B), safe] = 1.0 - float(smoothing)
        else:
            raise ValueError(kind)
        ignored = (cls == ignore_index) if ignore_index is not None else torch.zeros(B, dtype=torch.bool)
        cw = torch.ones(B, dtype=torch.float64) if w is None else w[safe]
    ss = S.sum(1)
    loss = cw * (lse * ss - (S * x).sum(1))
    grad = (go * cw)[:, None] * (torch.exp(x - lse[:, None]) * ss[:, None] - S)
    dead = bad | ignored
    loss = torch.where(bad, torch.full_like(loss, float("nan")), torch.where(ignored, torch.zeros_like(loss), loss))
    grad = torch.where(dead[:, None], torch.zeros_like(grad), grad)
    return loss, grad
