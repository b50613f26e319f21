"""CPU restatement of the fused optimizers under the non-finite guard (linnaeus_amd.optim, `nonfinite_guard=True`).

`GuardRef(kind, params, group)` is a `torch.optim.Optimizer` over CPU parameters whose `step()` is the clean update --
  adamw      torch.optim.AdamW (fp32)
  sgd        torch.optim.SGD (fp32)
  muon       tests/muon_ref.py (the restatement that tests/test_muon_fused_host.py pins to the reference bit for bit)
  ademamix   the fp64 restatement of tests/test_ademamix.py (parameters must be fp64)
-- and whose `skip()` is everything a skipped step does under the guard:
  * `state["step"] += 1` for adamw and ademamix (the host never learns of a skip, so the count is of ATTEMPTED steps; torch's own
    skipped step leaves it alone), the state created as the optimizer creates it when the parameter had none;
  * for sgd with momentum, a parameter without a momentum buffer gets a ZERO buffer (FusedSGD creates the buffer on the host before
    the kernel declines to fill it): the next step forms momentum 0 + (1 - dampening) g where torch clones g -- the same at dampening 0;
  * nothing else: no parameter, moment or momentum buffer changes, and Muon, which has no step-dependent term, does nothing at all.
Being an Optimizer, it can stand inside `torch.amp.GradScaler("cpu")` (tests/test_optim_guard_host.py).

`run(ref, grad_seq, poisoned)` drives one over a gradient sequence; a gradient of None leaves that parameter out of the step.
"""
import torch

from tests import muon_ref as R
from tests.test_ademamix import ref_init, ref_step

KINDS = ("adamw", "ademamix", "sgd", "muon")


class GuardRef(torch.optim.Optimizer):
    def __init__(self, kind, params, group):
        assert kind in KINDS, kind
        super().__init__(params, dict(group))
        self.kind = kind
        self.inner = None
        if kind in ("adamw", "sgd"):
            cls = torch.optim.AdamW if kind == "adamw" else torch.optim.SGD
            self.inner = cls([p for g in self.param_groups for p in g["params"]], **group)
        elif kind == "ademamix":
            assert all(p.dtype == torch.float64 for g in self.param_groups for p in g["params"]), "the AdEMAMix restatement is fp64"

    def state_of(self, p):
        return (self.inner if self.inner is not None else self).state[p]

    @torch.no_grad()
    def step(self, closure=None):
        assert closure is None
        if self.inner is not None:
            self.inner.step()
            return
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if self.kind == "muon":
                    new_p, st["momentum_buffer"], _ = R.step(p.detach(), p.grad, st.get("momentum_buffer"), group)
                    p.copy_(new_p)
                else:
                    if not st:
                        st.update(ref_init(p))
                    ref_step(p, p.grad, st, group)

    @torch.no_grad()
    def skip(self):
        """what is left of a step that the guard skipped"""
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state_of(p)
                if self.kind == "adamw":
                    if not st:  # as torch.optim.AdamW creates it
                        st["step"] = torch.tensor(0.0)
                        st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                    st["step"] += 1
                elif self.kind == "ademamix":
                    if not st:
                        st.update(ref_init(p))
                    st["step"] += 1
                elif self.kind == "sgd" and group["momentum"] != 0 and st.get("momentum_buffer") is None:
                    st["momentum_buffer"] = torch.zeros_like(p)


def run(ref, grad_seq, poisoned=()):
    """step s takes grad_seq[s] (one tensor or None per parameter, in group order); steps listed in `poisoned` are skipped"""
    params = [p for g in ref.param_groups for p in g["params"]]
    for s, grads in enumerate(grad_seq):
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.to(p.dtype).clone()
        if s in poisoned:
            ref.skip()
        else:
            ref.step()
    return params
