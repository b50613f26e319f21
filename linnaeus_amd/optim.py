"""Optimizer + step glue on device: `FusedAdamW` is a `torch.optim.Optimizer` whose
`step()` is one HIP launch for the whole model, three with clipping -- the sum of squares of every gradient (per-workgroup
partials + a fixed-order fold: bit-identical on every data-parallel rank), then a multi-tensor AdamW update with the
global-norm clip folded in (csrc/optim.hip) -- instead of `clip_grad_norm_` (the reference makes three
gradient passes with host syncs, train.py:282-308) followed by `torch.optim.AdamW.step`.

Same update rule and `param_groups` / `state_dict` layout as `torch.optim.AdamW` (per-group `lr`, `betas`, `eps`,
`weight_decay`; per-parameter `step`, `exp_avg`, `exp_avg_sq`), so LR schedulers and the reference's parameter-group
builder (optimizers/build.py) work unchanged.  GPU fp32 parameters only.

`FusedAdEMAMix` is the same machinery for the reference's AdEMAMix (optimizers/ademamix.py): one launch per step over the
same descriptor table plus a parallel table of slow-EMA pointers, three with the clip.  `FusedSGD` is torch.optim.SGD the same way,
`FusedMuon` the reference's Muon in a fixed number of launches.

`build_optimizer(config, model)` is the reference's optimizers/build.py with these classes, and `FusedMultiOptimizer` its
MultiOptimizer with the clip block of train.py:279-313 inside `step()`: one norm pass over every gradient of the run, the clip
coefficient applied by each sub-optimizer's kernel (`use_shared_clip`), nothing read back to the host.
"""
import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .loss import _cfg_get as _cfg, param_filter


def _slot_items(state, items, name):
    """[(param group, p)] -> ({(group, step): slot}, [(slot, p)]): one hyper-parameter slot per distinct (group, step count)"""
    slots = {}
    for gi, p in items:
        slots.setdefault((gi, int(state[p]["step"])), len(slots))
    if len(slots) > L.ADAMW_MAX_GROUPS:
        raise L.LnxError(f"{name}: {len(slots)} distinct (parameter group, step count) combinations, at most {L.ADAMW_MAX_GROUPS} are supported")
    return slots, [(slots[(gi, int(state[p]["step"]))], p) for gi, p in items]


def _adamw_descs(state, items):
    """host lnx_adamw_desc table of [(slot, p)] and its total workgroup count"""
    lib = L.lib()
    arr = (L.AdamWDesc * len(items))()
    blk = 0
    for i, (gi, p) in enumerate(items):  # gi: hyper-parameter slot = (param group, step count) combination
        st = state[p]
        arr[i].p, arr[i].m, arr[i].v, arr[i].g = p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.grad.data_ptr()
        arr[i].n, arr[i].group, arr[i].block_start = p.numel(), gi, blk
        blk += lib.lnx_adamw_blocks(C.c_int64(p.numel()))
    return arr, blk


def _grad_table(params, dev):
    """device lnx_adamw_desc table that carries only the gradients of `params` (all lnx_grad_sumsq reads), its length and workgroups"""
    lib = L.lib()
    arr = (L.AdamWDesc * len(params))()
    blk = 0
    for i, p in enumerate(params):
        arr[i].g, arr[i].n, arr[i].block_start = p.grad.data_ptr(), p.numel(), blk
        blk += lib.lnx_adamw_blocks(C.c_int64(p.numel()))
    return _upload(arr, dev), len(params), blk


def _upload(arr, dev):
    """a ctypes table on the device, through pinned memory when there is a GPU: the copy does not wait for the device"""
    host = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy())
    if dev.type != "cuda":
        return host
    host = host.pin_memory()
    out = host.to(dev, non_blocking=True)
    out._lnx_host = host  # pinned source stays alive as long as the table
    return out


class _SharedClip:
    """What the four fused optimizers share: `use_shared_clip(sumsq, max_norm)` hands the optimizer a device scalar with the sum of
    squares of ALL gradients of the run (FusedMultiOptimizer computes it once per step).  The optimizer then makes no norm pass of
    its own and its kernel clips by that scalar; `use_shared_clip(None)` restores its own behaviour."""

    _shared = None

    def use_shared_clip(self, sumsq: Optional[torch.Tensor], max_norm: Optional[float] = None):
        if sumsq is None:
            self._shared = None
            return
        if getattr(self, "max_grad_norm", None) is not None:
            raise ValueError(f"{type(self).__name__}: max_grad_norm is set; an optimizer clips either by its own norm or by a shared one")
        if not isinstance(sumsq, torch.Tensor) or sumsq.dtype != torch.float32 or sumsq.numel() != 1:
            raise ValueError("use_shared_clip: sumsq must be a one-element fp32 tensor")
        if max_norm is None or not max_norm > 0:
            raise ValueError(f"use_shared_clip: max_norm must be positive, got {max_norm}")
        self._shared = (sumsq, float(max_norm))

    def _clip(self, norm_pass):
        """(pointer of the sum of squares or None, max_norm) of this step; norm_pass() is run when the optimizer clips by itself"""
        if self._shared is not None:
            return self._shared[0].data_ptr(), self._shared[1]
        if self.max_grad_norm is not None and self.max_grad_norm > 0:
            norm_pass()
            return self._sumsq.data_ptr(), float(self.max_grad_norm)
        return None, 0.0


class FusedAdamW(_SharedClip, torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > L.ADAMW_MAX_GROUPS:
            raise ValueError(f"at most {L.ADAMW_MAX_GROUPS} parameter groups")
        self.max_grad_norm = max_grad_norm
        self._table = None
        self._key = None
        self._sumsq = None
        self._sumsq_ws = None

    # ------------------------------------------------------------------ descriptor table
    def _build(self, items):
        dev = items[0][1].device
        arr, blk = _adamw_descs(self.state, items)
        host = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy())
        self._table = (host.to(dev), len(items), blk)
        if self._sumsq is None or self._sumsq.device != dev:
            self._sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
        if self._sumsq_ws is None or self._sumsq_ws.device != dev or self._sumsq_ws.numel() < blk:
            self._sumsq_ws = torch.empty(blk, device=dev, dtype=torch.float32)  # one partial per workgroup (lnx_grad_sumsq: fixed-order fold)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        items = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise L.LnxError("FusedAdamW needs contiguous fp32 parameters and gradients on the GPU")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] = int(st["step"]) + 1  # int() also accepts the tensor a torch.optim.AdamW state_dict carries
                items.append((gi, p))
        if not items:
            return loss
        # torch.optim.AdamW bias-corrects PER PARAMETER (its own step count).  Parameters of one group normally share a
        # step count, but one that was frozen for a while, had no gradient on some steps or came from a checkpoint with
        # mixed steps does not: every distinct (group, step) pair gets its own hyper-parameter slot.
        slots, items = _slot_items(self.state, items, "FusedAdamW")
        key = tuple((si, p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr()) for si, p in items)
        if key != self._key:
            self._build(items)
            self._key = key
        h = L.AdamWHyper()
        h.ngroups = len(slots)
        for (gi, t), si in slots.items():
            group = self.param_groups[gi]
            b1, b2 = group["betas"]
            h.lr[si], h.beta1[si], h.beta2[si], h.eps[si], h.weight_decay[si] = group["lr"], b1, b2, group["eps"], group["weight_decay"]
            h.bias_c1[si], h.bias_c2[si] = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
            h.omb1[si], h.omb2[si] = 1.0 - b1, 1.0 - b2
        table, n, blocks = self._table
        lib = L.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        sumsq, max_norm = self._clip(lambda: L.check(
            lib.lnx_grad_sumsq(C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self._sumsq.data_ptr()), C.c_void_p(self._sumsq_ws.data_ptr()), stream), "lnx_grad_sumsq"))
        L.check(lib.lnx_adamw_step(C.c_void_p(table.data_ptr()), n, blocks, C.byref(h), C.c_void_p(sumsq), C.c_float(max_norm), stream), "lnx_adamw_step")
        return loss

    def grad_norm(self) -> Optional[torch.Tensor]:
        """total L2 norm of the gradients seen by the last clipped step (device scalar, no sync); None without clipping"""
        if self._sumsq is None or self.max_grad_norm is None:
            return None
        return self._sumsq.sqrt()[0]


def ademamix_schedule(step: int, alpha: float, beta1: float, beta3: float, T_alpha_beta3: Optional[float]):
    """(alpha_t, beta3_t) of AdEMAMix at a parameter's step (1-based), in double: alpha warms up linearly over T steps,
    beta3 follows the log-interpolation from beta1 (Pagliardini et al. 2024), both capped at their final values.  Without T
    they are constant."""
    if T_alpha_beta3 is None:
        return float(alpha), float(beta3)
    f = step / T_alpha_beta3
    lb1, lb3 = math.log(beta1), math.log(beta3)
    return min(step * alpha / T_alpha_beta3, alpha), min(math.exp(lb1 * lb3 / ((1.0 - f) * lb3 + f * lb1)), beta3)


def _check_ademamix_group(lr, betas, eps, weight_decay, T_alpha_beta3):
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if len(betas) != 3 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"Invalid beta parameters: {betas}, expected three in [0, 1)")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if T_alpha_beta3 is not None:
        # the reference only fails on these at its first step (a division by zero, or log(0) in the beta3 schedule)
        if not T_alpha_beta3 > 0:
            raise ValueError(f"Invalid T_alpha_beta3 value: {T_alpha_beta3} (must be > 0, or None)")
        if betas[0] == 0.0 or betas[2] == 0.0:
            raise ValueError(f"Invalid beta parameters: {betas}: the T_alpha_beta3 schedule needs beta1 > 0 and beta3 > 0")


class FusedAdEMAMix(_SharedClip, torch.optim.Optimizer):
    """AdEMAMix (linnaeus/optimizers/ademamix.py, chosen by OPTIMIZER.NAME = ademamix in optimizers/build.py) as one
    multi-tensor HIP launch per step, three with clipping (lnx_grad_sumsq, then lnx_ademamix_step with the clip folded in),
    instead of the reference's ~13 tensor ops per parameter.

    Same constructor defaults, `param_groups` keys (lr, betas, eps, weight_decay, alpha, T_alpha_beta3) and per-parameter
    state (step, exp_avg, exp_avg_sq, exp_avg_slow) as the reference, so its checkpoints load with `load_state_dict` and
    the other way round, and LR schedulers and build.py's parameter groups work unchanged.  The update is the reference's,
    including its quirk of dividing the slow EMA by the first bias correction as well (csrc/optim.hip).

    `max_grad_norm` clips over THIS optimizer's parameters.  When linnaeus builds one optimizer per parameter group
    (PARAMETER_GROUPS.ENABLED), leave it None and clip once, over all parameters, before the steps: `FusedMultiOptimizer`
    does that on the device through `use_shared_clip`.  GPU fp32 only.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999, 0.9999), eps: float = 1e-8, weight_decay: float = 0, alpha: float = 5.0,
                 T_alpha_beta3: Optional[float] = None, max_grad_norm: Optional[float] = None):
        _check_ademamix_group(lr, betas, eps, weight_decay, T_alpha_beta3)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, alpha=alpha, T_alpha_beta3=T_alpha_beta3))
        for g in self.param_groups:  # groups may carry their own values
            _check_ademamix_group(g["lr"], g["betas"], g["eps"], g["weight_decay"], g["T_alpha_beta3"])
        if len(self.param_groups) > L.ADAMW_MAX_GROUPS:
            raise ValueError(f"at most {L.ADAMW_MAX_GROUPS} parameter groups")
        self.max_grad_norm = max_grad_norm
        self._table = None
        self._key = None
        self._sumsq = None
        self._sumsq_ws = None

    def _build(self, items):
        dev = items[0][1].device
        for _, p in items:  # the kernel indexes every state tensor with the parameter's offsets
            for k in ("exp_avg", "exp_avg_sq", "exp_avg_slow"):
                t = self.state[p][k]
                if t.device != dev or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous():
                    raise L.LnxError(f"FusedAdEMAMix: state '{k}' must be a contiguous fp32 tensor of the parameter's shape on its device")
        arr, blk = _adamw_descs(self.state, items)
        slow = (C.c_uint64 * len(items))(*(self.state[p]["exp_avg_slow"].data_ptr() for _, p in items))
        descs = np.frombuffer(arr, dtype=np.uint8)
        host = torch.from_numpy(np.concatenate([descs, np.frombuffer(slow, dtype=np.uint8)]))  # one copy: descriptors, then slow pointers
        self._table = (host.to(dev), len(descs), len(items), blk)
        if self._sumsq is None or self._sumsq.device != dev:
            self._sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
        if self._sumsq_ws is None or self._sumsq_ws.device != dev or self._sumsq_ws.numel() < blk:
            self._sumsq_ws = torch.empty(blk, device=dev, dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        items = []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise L.LnxError("FusedAdEMAMix needs contiguous fp32 parameters and gradients on the GPU")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_slow"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] = int(st["step"]) + 1  # int() also accepts a tensor step
                items.append((gi, p))
        if not items:
            return loss
        # bias corrections, alpha_t and beta3_t all follow each parameter's own step count (as in the reference)
        slots, items = _slot_items(self.state, items, "FusedAdEMAMix")
        key = tuple((si, p.data_ptr(), p.grad.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr(),
                     self.state[p]["exp_avg_slow"].data_ptr()) for si, p in items)
        if key != self._key:
            self._build(items)
            self._key = key
        h = L.AdEMAMixHyper()
        h.ngroups = len(slots)
        for (gi, t), si in slots.items():
            group = self.param_groups[gi]
            b1, b2, b3 = group["betas"]
            alpha_t, beta3_t = ademamix_schedule(t, group["alpha"], b1, b3, group["T_alpha_beta3"])
            h.lr[si], h.beta1[si], h.beta2[si], h.eps[si], h.weight_decay[si] = group["lr"], b1, b2, group["eps"], group["weight_decay"]
            h.bias_c1[si], h.bias_c2[si] = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
            h.omb1[si], h.omb2[si] = 1.0 - b1, 1.0 - b2
            h.alpha_t[si], h.beta3_t[si], h.omb3[si] = alpha_t, beta3_t, 1.0 - beta3_t
        table, nbytes, n, blocks = self._table
        lib = L.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        sumsq, max_norm = self._clip(lambda: L.check(
            lib.lnx_grad_sumsq(C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self._sumsq.data_ptr()), C.c_void_p(self._sumsq_ws.data_ptr()), stream), "lnx_grad_sumsq"))
        L.check(lib.lnx_ademamix_step(table.data_ptr(), table.data_ptr() + nbytes, n, blocks, C.byref(h), sumsq, max_norm, stream), "lnx_ademamix_step")
        return loss

    def grad_norm(self) -> Optional[torch.Tensor]:
        """total L2 norm of the gradients seen by the last clipped step (device scalar, no sync); None without clipping"""
        if self._sumsq is None or self.max_grad_norm is None:
            return None
        return self._sumsq.sqrt()[0]


# ----------------------------------------------------------------------------------------------------------------------
# Muon: SGD-momentum whose 2-D update is orthogonalised by five Newton-Schulz iterations in bf16
# (optimizers/muon.py:27-65, 67-160).  The 15 matrix products per parameter run on lnx_gemm_nt (bf16 MFMA, fp32
# accumulate): A = X X^T, B = c A A + b A and X' = B X + a X are each ONE launch (the affine terms ride in the GEMM
# epilogue as the per-column scale and the fp32 residual), where the reference issues a matmul plus elementwise
# bf16 passes per term.  Same constructor, param_groups and state ('momentum_buffer') as the reference's Muon.
# ----------------------------------------------------------------------------------------------------------------------
def zeropower_via_newtonschulz5(G: torch.Tensor, steps: int = 5) -> torch.Tensor:
    """Orthogonalise a 2-D gradient (quintic Newton-Schulz, coefficients of optimizers/muon.py:41).  bf16 in / out."""
    from . import ops

    assert G.ndim == 2, "2-D matrices (4-D conv weights are flattened by the optimizer)"
    if not G.is_cuda:
        raise L.LnxError("linnaeus_amd.optim.Muon runs on the HIP GEMM kernels: parameters must be on the GPU")
    a, b, c = 3.4445, -4.7750, 2.0315
    X = G.bfloat16()
    tall = G.size(0) > G.size(1)
    if tall:
        X = X.t()
    m, n = X.shape
    mp, npad = (m + 7) // 8 * 8, (n + 7) // 8 * 8   # GEMM K granularity; zero rows / columns do not change any product
    X = X / (X.float().norm() + 1e-7).to(torch.bfloat16)
    if (mp, npad) != (m, n):
        X = torch.nn.functional.pad(X, (0, npad - n, 0, mp - m))
    X = X.contiguous()
    dev = X.device
    cvec = torch.full((mp,), c, device=dev, dtype=torch.float32)
    ones = None
    A = torch.empty(mp, mp, device=dev, dtype=torch.bfloat16)
    Bm = torch.empty(mp, mp, device=dev, dtype=torch.bfloat16)
    Xn = torch.empty(mp, npad, device=dev, dtype=torch.bfloat16)
    for _ in range(steps):
        XT = X.t().contiguous()                                   # [n, m]: the "W" operand of B . X
        ops.gemm_nt(X, X, A)                                      # A = X X^T
        ops.gemm_nt(A, A, Bm, gamma=cvec, res=A.float() * b)      # B = c A A + b A   (A symmetric: A A^T = A A)
        ops.gemm_nt(Bm, XT, Xn, res=X.float() * a)                # X' = B X + a X
        X, Xn = Xn, X
    X = X[:m, :n]
    return (X.t() if tall else X).contiguous()


class Muon(torch.optim.Optimizer):
    """optimizers/muon.py:67-160 on the HIP kernels (2-D parameters, or 4-D conv weights flattened to [out, -1])."""

    def __init__(self, params, lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5, strict=False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        params = list(params)
        if strict:
            for p in (q for g in params for q in (g["params"] if isinstance(g, dict) else [g])):
                if p.dim() not in (2, 4):
                    raise ValueError(f"Muon optimizer requires 2D or 4D parameters, got shape {p.shape}")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov, ns_steps=ns_steps))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr, wd, mom = group["lr"], group["weight_decay"], group["momentum"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = p.grad
                if wd != 0:
                    p.mul_(1 - lr * wd)
                st = self.state[p]
                if "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros_like(g)
                buf = st["momentum_buffer"]
                buf.lerp_(g, 1 - mom)
                g = g.lerp_(buf, mom) if group["nesterov"] else buf.clone()
                g2 = g.view(g.size(0), -1) if g.ndim == 4 else g
                o = zeropower_via_newtonschulz5(g2, steps=group["ns_steps"])
                if p.dim() == 4:
                    scaling = max(1, p.size(0) / (p.size(1) * p.size(2) * p.size(3))) ** 0.5
                else:
                    scaling = max(1, p.size(-2) / p.size(-1)) ** 0.5
                p.add_(o.view_as(p).to(p.dtype), alpha=-lr * scaling)
        return loss


def muon_layout(shapes):
    """lnx_muon_layout of a list of logical [rows, cols] shapes (host only, no GPU): (MuonMat array, tile table as an int32 array
    [ntiles, 4] = (matrix, tile row, tile column, 0) with the three stage tables one after the other, MuonInfo)."""
    lib = L.lib()
    n = len(shapes)
    flat = (C.c_int * (2 * max(n, 1)))(*(int(v) for s in shapes for v in s))
    mats = (L.MuonMat * max(n, 1))()
    info = L.MuonInfo()
    L.check(lib.lnx_muon_layout(flat, n, mats, None, 0, C.byref(info)), "lnx_muon_layout")
    tiles = np.zeros((sum(info.ntiles), 4), dtype=np.int32)
    L.check(lib.lnx_muon_layout(flat, n, mats, tiles.ctypes.data, tiles.shape[0], C.byref(info)), "lnx_muon_layout")
    return mats, tiles, info


def muon_parameters(model):
    """the parameters optimizers/build.py:130-154 hands to Muon: trainable, 2-D or 4-D, and no 'embed', 'token', 'head' or
    'classifier' in the name (those, and every other shape, go to AdamW)"""
    return [p for name, p in model.named_parameters()
            if p.requires_grad and p.dim() in (2, 4) and not any(k in name.lower() for k in ("embed", "token", "cls_token", "head", "classifier"))]


def _muon_shape(p):
    return (p.size(0), p.numel() // p.size(0))


class FusedMuon(_SharedClip, torch.optim.Optimizer):
    """Muon (linnaeus/optimizers/muon.py:67-190, OPTIMIZER.NAME = muon) as 3 * max(ns_steps) + 3 HIP launches per step for ALL matrices
    together (csrc/muon.hip): momentum and Nesterov, normalisation, the Newton-Schulz products as grouped bf16 MFMA launches, and
    the update, instead of the ~50 launches per parameter of `Muon` above.

    Same constructor, `param_groups` keys (lr, weight_decay, momentum, nesterov, ns_steps) and per-parameter state
    (`momentum_buffer`, fp32) as the reference and as `Muon`, so checkpoints move between the three with `load_state_dict`.
    Groups may differ in every hyper-parameter; a parameter whose `.grad` is None is skipped for the step (no decay, no state).
    Differences from the reference:
      * parameters that are not 2-D or 4-D raise ValueError at construction whatever `strict` says (the reference fails inside
        its first step);
      * `.grad` is left untouched (the reference overwrites it with the Nesterov gradient, muon.py:167);
      * each product is rounded to bf16 once, after its affine term, as `zeropower_via_newtonschulz5` above does.
    `max_grad_norm` clips by the global norm of THIS optimizer's gradients (one lnx_grad_sumsq pass, two more launches), the clip
    coefficient multiplying each gradient element as the momentum kernel reads it; `use_shared_clip` takes the norm of a whole run
    from `FusedMultiOptimizer` instead.  Contiguous fp32 parameters and gradients on the GPU only.  Bit-reproducible: no atomics, the same inputs give the same
    parameters whatever else is in the optimizer, so data-parallel replicas that each run the whole step stay equal.
    """

    def __init__(self, params, lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5, strict=False, max_grad_norm: Optional[float] = None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= momentum < 1.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if int(ns_steps) != ns_steps or ns_steps < 0:
            raise ValueError(f"Invalid ns_steps value: {ns_steps}")
        super().__init__(params, dict(lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov, ns_steps=ns_steps))
        for g in self.param_groups:
            for p in g["params"]:
                if p.dim() not in (2, 4):
                    raise ValueError(f"Muon optimizer requires 2D or 4D parameters, got shape {p.shape}")
        self._key = None      # what the layout depends on: shapes and ns_steps in launch order
        self._order = None    # [(group index, p)] by descending ns_steps: each iteration launches a prefix of the tile tables
        self._mats = None     # host lnx_muon_mat table
        self._sent = None     # bytes of the table as last copied to the device
        self._dev = None      # (device table, device tile tables, workspace, partials, MuonInfo)
        self.max_grad_norm = max_grad_norm
        self._sumsq = None    # own clip: sum of squares of this optimizer's gradients ...
        self._gtable = None   # ... over a gradient-only descriptor table (key, table, n, blocks, partials)

    def _build(self, order, dev):
        mats, tiles, info = muon_layout([_muon_shape(p) for _, p in order])
        self._mats = mats
        self._dev = (torch.empty(C.sizeof(mats), device=dev, dtype=torch.uint8), torch.from_numpy(tiles).to(dev),
                     torch.zeros(info.workspace_bytes, device=dev, dtype=torch.uint8),  # zero-filled once: the padding stays zero
                     torch.empty(info.total_blocks, device=dev, dtype=torch.float32), info)
        self._sent = None

    def workspace_bytes(self) -> int:
        """bytes of the bf16 workspace of the last step's layout (0 before the first step)"""
        return 0 if self._dev is None else int(self._dev[4].workspace_bytes)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        order = [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        if not order:
            return loss
        for gi, g in enumerate(self.param_groups):
            if int(g["ns_steps"]) != g["ns_steps"] or g["ns_steps"] < 0:
                raise ValueError(f"Invalid ns_steps value: {g['ns_steps']}")
        order.sort(key=lambda it: -int(self.param_groups[it[0]]["ns_steps"]))  # stable: ties keep the parameter order
        with_grad = [p for _, p in order if p.grad is not None]
        if not with_grad:
            return loss
        dev = with_grad[0].device
        for p in with_grad:  # a parameter without a gradient is not touched this step
            if not p.is_cuda or p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise L.LnxError("FusedMuon needs contiguous fp32 parameters on one GPU")
            if p.grad.device != dev or p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.shape != p.shape:
                raise L.LnxError("FusedMuon needs contiguous fp32 gradients on the parameters' GPU")
        key = tuple((id(p), tuple(p.shape), int(self.param_groups[gi]["ns_steps"])) for gi, p in order)
        if key != self._key:
            self._build(order, dev)
            self._key, self._order = key, order
        mats = self._mats
        for i, (gi, p) in enumerate(order):
            g, m = self.param_groups[gi], mats[i]
            m.p = p.data_ptr()
            if p.grad is None:
                m.g = m.buf = None
            else:
                st = self.state[p]
                if "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros_like(p.grad)
                buf = st["momentum_buffer"]
                if buf.device != dev or buf.dtype != torch.float32 or buf.shape != p.shape or not buf.is_contiguous():
                    raise L.LnxError("FusedMuon: state 'momentum_buffer' must be a contiguous fp32 tensor of the parameter's shape on its device")
                m.g, m.buf = p.grad.data_ptr(), buf.data_ptr()
            rows, cols = _muon_shape(p)
            lr, mom = float(g["lr"]), float(g["momentum"])
            m.ns_steps, m.nesterov = int(g["ns_steps"]), 1 if g["nesterov"] else 0
            m.momentum, m.omm = mom, 1 - mom
            m.decay, m.step = 1 - lr * float(g["weight_decay"]), lr * max(1, rows / cols) ** 0.5
        table, tiles, ws, part, info = self._dev
        raw = bytes(mats)
        if raw != self._sent:  # gradient pointers and learning rates usually move between steps; the layout does not
            table.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            self._sent = raw
        a = L.MuonStepArgs()
        a.n, a.mats, a.mats_dev, a.tiles_dev = len(order), C.addressof(mats), table.data_ptr(), tiles.data_ptr()
        a.workspace, a.workspace_bytes, a.partials = ws.data_ptr(), ws.numel(), part.data_ptr()
        a.sumsq, a.max_norm = self._clip(lambda: self._norm_pass(with_grad, dev))
        L.check(L.lib().lnx_muon_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_muon_step")
        return loss

    def _norm_pass(self, with_grad, dev):
        key = tuple(p.grad.data_ptr() for p in with_grad)
        if self._gtable is None or self._gtable[0] != key:
            table, n, blocks = _grad_table(with_grad, dev)
            self._gtable = (key, table, n, blocks, torch.empty(blocks, device=dev, dtype=torch.float32))
        if self._sumsq is None or self._sumsq.device != dev:
            self._sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
        _, table, n, blocks, ws = self._gtable
        L.check(L.lib().lnx_grad_sumsq(C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self._sumsq.data_ptr()), C.c_void_p(ws.data_ptr()),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_grad_sumsq")

    def grad_norm(self) -> Optional[torch.Tensor]:
        """total L2 norm of the gradients seen by the last clipped step (device scalar, no sync); None without clipping"""
        if self._sumsq is None or self.max_grad_norm is None:
            return None
        return self._sumsq.sqrt()[0]


# ----------------------------------------------------------------------------------------------------------------------
# SGD (OPTIMIZER.NAME = sgd; optimizers/build.py always builds it with nesterov=True): torch.optim.SGD's update as one launch
# ----------------------------------------------------------------------------------------------------------------------
class FusedSGD(_SharedClip, torch.optim.Optimizer):
    """`torch.optim.SGD` as one multi-tensor HIP launch per step (lnx_sgd_step), three with clipping, instead of torch's foreach
    passes.  Same `param_groups` keys and per-parameter state (`momentum_buffer`) as `torch.optim.SGD`, so state dicts load both
    ways; a missing or None buffer means "first step for this parameter" (the buffer then starts as the decayed gradient, as in
    torch).  One hyper-parameter slot per distinct (group, first step or not) pair.  `maximize=True` is refused, as is whatever
    torch's constructor refuses (Nesterov without momentum or with dampening, negative values).  A parameter without `.grad` is
    skipped.  `max_grad_norm` clips over THIS optimizer's parameters; `use_shared_clip` takes a run's norm instead.  GPU fp32 only.
    """

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0, dampening: float = 0, weight_decay: float = 0, nesterov: bool = False,
                 max_grad_norm: Optional[float] = None):
        # torch's own constructor checks and its group keys (maximize, foreach, differentiable, fused, ...), whatever the torch version
        defaults = dict(torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov).defaults)
        super().__init__(params, defaults)
        for g in self.param_groups:
            self._check_group(g)
        if len(self.param_groups) > L.ADAMW_MAX_GROUPS // 2:
            raise ValueError(f"at most {L.ADAMW_MAX_GROUPS // 2} parameter groups (two hyper-parameter slots each)")
        self.max_grad_norm = max_grad_norm
        self._table = None
        self._key = None
        self._sumsq = None
        self._sumsq_ws = None

    @staticmethod
    def _check_group(g):
        if g.get("maximize"):
            raise ValueError("FusedSGD does not support maximize=True")
        if isinstance(g["lr"], torch.Tensor):
            raise ValueError("FusedSGD needs a float lr")
        if g["lr"] < 0.0:
            raise ValueError(f"Invalid learning rate: {g['lr']}")
        if g["momentum"] < 0.0:
            raise ValueError(f"Invalid momentum value: {g['momentum']}")
        if g["weight_decay"] < 0.0:
            raise ValueError(f"Invalid weight_decay value: {g['weight_decay']}")
        if g["nesterov"] and (g["momentum"] <= 0 or g["dampening"] != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        items, slots = [], {}
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)  # a loaded state dict or a scheduler may have changed it
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                    raise L.LnxError("FusedSGD needs contiguous fp32 parameters and gradients on the GPU")
                buf, first = None, False
                if group["momentum"] != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    first = buf is None
                    if first:
                        buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.preserve_format)  # the kernel writes all of it
                    elif buf.device != p.device or buf.dtype != torch.float32 or buf.shape != p.shape or not buf.is_contiguous():
                        raise L.LnxError("FusedSGD: state 'momentum_buffer' must be a contiguous fp32 tensor of the parameter's shape on its device")
                items.append((slots.setdefault((gi, first), len(slots)), p, buf))
        if not items:
            return loss
        key = tuple((si, p.data_ptr(), p.grad.data_ptr(), 0 if buf is None else buf.data_ptr()) for si, p, buf in items)
        if key != self._key:
            dev = items[0][1].device
            lib = L.lib()
            arr = (L.AdamWDesc * len(items))()
            blk = 0
            for i, (si, p, buf) in enumerate(items):
                arr[i].p, arr[i].m, arr[i].g = p.data_ptr(), None if buf is None else buf.data_ptr(), p.grad.data_ptr()
                arr[i].n, arr[i].group, arr[i].block_start = p.numel(), si, blk
                blk += lib.lnx_adamw_blocks(C.c_int64(p.numel()))
            self._table = (_upload(arr, dev), len(items), blk)
            if self._sumsq is None or self._sumsq.device != dev:
                self._sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
            if self._sumsq_ws is None or self._sumsq_ws.device != dev or self._sumsq_ws.numel() < blk:
                self._sumsq_ws = torch.empty(blk, device=dev, dtype=torch.float32)
            self._key = key
        h = L.SGDHyper()
        h.ngroups = len(slots)
        for (gi, first), si in slots.items():
            g = self.param_groups[gi]
            h.lr[si], h.momentum[si], h.dampening[si], h.weight_decay[si] = g["lr"], g["momentum"], g["dampening"], g["weight_decay"]
            h.nesterov[si], h.first[si] = 1 if g["nesterov"] else 0, 1 if first else 0
        table, n, blocks = self._table
        lib = L.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        sumsq, max_norm = self._clip(lambda: L.check(
            lib.lnx_grad_sumsq(C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self._sumsq.data_ptr()), C.c_void_p(self._sumsq_ws.data_ptr()), stream), "lnx_grad_sumsq"))
        L.check(lib.lnx_sgd_step(table.data_ptr(), n, blocks, C.byref(h), sumsq, max_norm, stream), "lnx_sgd_step")
        return loss

    def grad_norm(self) -> Optional[torch.Tensor]:
        """total L2 norm of the gradients seen by the last clipped step (device scalar, no sync); None without clipping"""
        if self._sumsq is None or self.max_grad_norm is None:
            return None
        return self._sumsq.sqrt()[0]


# ----------------------------------------------------------------------------------------------------------------------
# The configured optimizer (optimizers/build.py + optimizers/multi_optimizer.py + the clip block of train.py:279-313)
# ----------------------------------------------------------------------------------------------------------------------
FUSED_OPTIMIZERS = (FusedAdamW, FusedAdEMAMix, FusedSGD, FusedMuon)


class FusedMultiOptimizer:
    """The reference's `MultiOptimizer` (same interface: `optimizers`, `param_groups` carrying `optimizer_name` /
    `optimizer_group_idx`, `step`, `zero_grad`, `add_param_group`, `state_dict`, `load_state_dict`) with the gradient clip of
    train.py:279-313 inside `step()`: with `max_grad_norm`, ONE lnx_grad_sumsq pass (two launches, fixed-order fold) over every
    gradient of every sub-optimizer, then every sub-optimizer steps with that device scalar (`use_shared_clip`): its kernel
    scales the gradients as it reads them.  Nothing is read back to the host.

    The union table lists the parameters by SORTED optimizer name, then group, then position in the group -- the order of the
    stable state-dict indices -- so the norm's bits do not depend on the order the optimizers were inserted in.  It is rebuilt
    only when a gradient pointer changes.  `.grad` is left as it was (clip_grad_norm_ scales it in place).

    Refused: a sub-optimizer with its own `max_grad_norm`; with a clip, a sub-optimizer that is not FusedAdamW, FusedAdEMAMix,
    FusedSGD or FusedMuon; a parameter held by two sub-optimizers (the reference would step it twice).

    `state_dict()` writes the layout the reference's code intends but does not produce (its saved per-optimizer "state" is always
    empty): `_version` 2, `_param_shapes`, `optimizers[name] = {"state": {stable index: ...}, "param_groups"}`.
    """

    def __init__(self, optimizers: dict, max_grad_norm: Optional[float] = None):
        self.optimizers = optimizers
        self.max_grad_norm = None if max_grad_norm is None or not max_grad_norm > 0 else float(max_grad_norm)
        seen = {}
        for name, opt in optimizers.items():
            if getattr(opt, "max_grad_norm", None) is not None:
                raise ValueError(f"FusedMultiOptimizer: sub-optimizer '{name}' has its own max_grad_norm; the clip is global, set it on the multi-optimizer")
            if self.max_grad_norm is not None and not isinstance(opt, FUSED_OPTIMIZERS):
                raise ValueError(f"FusedMultiOptimizer: sub-optimizer '{name}' ({type(opt).__name__}) is not a fused optimizer; "
                                 "the shared clip needs FusedAdamW, FusedAdEMAMix, FusedSGD or FusedMuon")
            for group in opt.param_groups:
                for p in group["params"]:
                    if id(p) in seen:
                        raise ValueError(f"FusedMultiOptimizer: a parameter of shape {tuple(p.shape)} is held by both '{seen[id(p)]}' and '{name}'")
                    seen[id(p)] = name
        self.param_groups = []
        for name, opt in optimizers.items():
            for i, group in enumerate(opt.param_groups):
                group["optimizer_name"] = name
                group["optimizer_group_idx"] = i
                self.param_groups.append(group)
        self._sumsq = None
        self._union = None  # (key, device table, n, blocks, partials)

    # ------------------------------------------------------------------ step
    def _ordered_params(self):
        """every parameter in stable order: sorted optimizer name, group, position"""
        return [p for name in sorted(self.optimizers) for g in self.optimizers[name].param_groups for p in g["params"]]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.max_grad_norm is not None:
            with_grad = [p for p in self._ordered_params() if p.grad is not None]
            if with_grad:
                dev = with_grad[0].device
                for p in with_grad:
                    if not p.grad.is_cuda or p.grad.device != dev or p.grad.dtype != torch.float32 or not p.grad.is_contiguous():
                        raise L.LnxError("FusedMultiOptimizer needs contiguous fp32 gradients on one GPU")
                key = tuple((p.grad.data_ptr(), p.numel()) for p in with_grad)
                if self._union is None or self._union[0] != key:
                    table, n, blocks = _grad_table(with_grad, dev)
                    self._union = (key, table, n, blocks, torch.empty(blocks, device=dev, dtype=torch.float32))
                if self._sumsq is None or self._sumsq.device != dev:
                    self._sumsq = torch.zeros(1, device=dev, dtype=torch.float32)
                _, table, n, blocks, ws = self._union
                L.check(L.lib().lnx_grad_sumsq(C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self._sumsq.data_ptr()), C.c_void_p(ws.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_grad_sumsq")
                for opt in self.optimizers.values():
                    opt.use_shared_clip(self._sumsq, self.max_grad_norm)
        for opt in self.optimizers.values():
            opt.step()
        return loss

    def grad_norm(self) -> Optional[torch.Tensor]:
        """pre-clip L2 norm of all gradients of the last step (device scalar, no sync); None without clipping or before a step"""
        if self._sumsq is None or self.max_grad_norm is None:
            return None
        return self._sumsq.sqrt()[0]

    def grad_norms(self):
        """(pre-clip norm, post-clip norm, the value clip_grad_norm_ returned) of the last step, the three values train.py:339-348
        logs, as device scalars.  The post-clip norm is pre * coef with the kernels' coef = min(1, max / (pre + 1e-6)); the reference
        measures the clipped gradients again.  The third equals the first."""
        pre = self.grad_norm()
        if pre is None:
            return None
        coef = torch.clamp(self.max_grad_norm / (pre + 1e-6), max=1.0)
        return pre, pre * coef, pre

    def zero_grad(self, set_to_none: bool = False) -> None:
        for opt in self.optimizers.values():
            opt.zero_grad(set_to_none=set_to_none)

    def add_param_group(self, param_group: dict) -> None:
        if "optimizer_name" not in param_group:
            raise ValueError("param_group must include 'optimizer_name' key")
        name = param_group.pop("optimizer_name")
        if name not in self.optimizers:
            raise ValueError(f"Optimizer '{name}' not found")
        held = {id(p) for p in self._ordered_params()}
        new = param_group["params"]
        for p in [new] if isinstance(new, torch.Tensor) else list(new):
            if id(p) in held:
                raise ValueError(f"FusedMultiOptimizer: a parameter of shape {tuple(p.shape)} is already held by a sub-optimizer")
        opt = self.optimizers[name]
        opt.add_param_group(param_group)
        group = opt.param_groups[-1]
        group["optimizer_name"] = name
        group["optimizer_group_idx"] = len(opt.param_groups) - 1
        self.param_groups.append(group)

    # ------------------------------------------------------------------ state
    def _bases(self):
        """first stable index of every sub-optimizer"""
        bases, n = {}, 0
        for name in sorted(self.optimizers):
            bases[name] = n
            n += sum(len(g["params"]) for g in self.optimizers[name].param_groups)
        return bases

    def state_dict(self) -> dict:
        bases = self._bases()
        out = {"_version": 2, "_param_shapes": [tuple(p.shape) for p in self._ordered_params()], "optimizers": {}}
        for name, opt in self.optimizers.items():
            sd = opt.state_dict()  # torch packs the parameters 0, 1, ... in group order: the stable index is that plus the optimizer's base
            out["optimizers"][name] = {"state": {bases[name] + int(k): v for k, v in sd["state"].items()}, "param_groups": sd["param_groups"]}
        return out

    def load_state_dict(self, state_dict: dict) -> None:
        import warnings

        if state_dict.get("_version", 1) == 1:  # legacy: {name: opt.state_dict()}
            for name, opt in self.optimizers.items():
                if name in state_dict:
                    opt.load_state_dict(state_dict[name])
                else:
                    warnings.warn(f"FusedMultiOptimizer: no state for optimizer '{name}' in the state dict")
            return
        shapes = [tuple(s) for s in state_dict.get("_param_shapes", [])]
        mine = [tuple(p.shape) for p in self._ordered_params()]
        if shapes and shapes != mine:
            raise ValueError("FusedMultiOptimizer: the state dict was written for other parameters (_param_shapes differ)")
        bases = self._bases()
        saved = state_dict.get("optimizers", {})
        if saved and all(len(s.get("state", {})) == 0 for s in saved.values()):
            warnings.warn("FusedMultiOptimizer: the state dict holds no optimizer state (the reference's MultiOptimizer writes such files); "
                          "starting from fresh state")
        for name, opt in self.optimizers.items():
            if name not in saved:
                warnings.warn(f"FusedMultiOptimizer: no state for optimizer '{name}' in the state dict")
                continue
            count = sum(len(g["params"]) for g in opt.param_groups)
            state = {}
            for k, v in saved[name]["state"].items():
                i = int(k) - bases[name]
                if not 0 <= i < count:
                    raise ValueError(f"FusedMultiOptimizer: stable index {k} does not belong to optimizer '{name}'")
                state[i] = v
            opt.load_state_dict({"state": state, "param_groups": saved[name]["param_groups"]})

    def __repr__(self) -> str:
        return self.__class__.__name__ + " (\n" + "".join(f"  {name}: {opt.__class__.__name__},\n" for name, opt in self.optimizers.items()) + ")"


MUON_SKIP_KEYWORDS = ("embed", "token", "cls_token", "head", "classifier")  # optimizers/build.py:135-138: these go to AdamW
_UNKNOWN_FILTERS = ("convolutional", "layer_type", "initialization", "stage_based")


def _check_filter_types(spec, group):
    kind = str(_cfg(spec, "TYPE", "")).lower()
    if kind in _UNKNOWN_FILTERS:
        raise ValueError(f"build_optimizer: filter type '{kind}' (parameter group {group}) is not supported; supported: name, dimension, and, or, not, all_except")
    for sub in list(_cfg(spec, "FILTERS", [])) + [x for x in (_cfg(spec, "FILTER", None), _cfg(spec, "EXCEPT", None)) if x is not None]:
        _check_filter_types(sub, group)


def set_weight_decay(model, skip_list=(), skip_keywords=()):
    """optimizers/build.py:687-716: [decay group, no-decay group (1-D, *.bias, the model's no_weight_decay names / keywords)]"""
    has_decay, no_decay = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if p.dim() == 1 or name.endswith(".bias") or name in skip_list or any(k in name for k in skip_keywords):
            no_decay.append(p)
        else:
            has_decay.append(p)
    return [{"params": has_decay}, {"params": no_decay, "weight_decay": 0.0}]


def build_optimizer(config, model, max_grad_norm="config", freeze_4d_like_reference: bool = False):
    """optimizers/build.py's `build_optimizer`, branch for branch, with the fused classes: `OPTIMIZER.NAME` sgd / adamw / ademamix over
    the decay / no-decay split; muon as {"MUON": FusedMuon, "ADAMW": FusedAdamW}; and with `OPTIMIZER.PARAMETER_GROUPS.ENABLED` one
    optimizer per group (filters of `loss.param_filter`, `LR_MULTIPLIER`, `WEIGHT_DECAY`, `{group}_ADAMW` for the non-matrix parameters
    of a Muon group, `DEFAULT` / `DEFAULT_MUON` / `DEFAULT_ADAMW` for the unmatched ones, in named_parameters() order where the reference
    iterates a set).  Missing config nodes take the reference config.py's defaults.

    max_grad_norm: "config" reads TRAIN.CLIP_GRAD (default 5.0); None or <= 0: no clip.  A single optimizer gets it as its own
    `max_grad_norm`, several get it through `FusedMultiOptimizer`: either way the clip of train.py:279-313 is inside `step()`.
    4-D parameters selected for Muon are trained.  The reference never updates them (it hands Muon wrappers whose .grad stays None):
    freeze_4d_like_reference=True leaves them out of every optimizer, which is what the reference effectively does.
    """
    if max_grad_norm == "config":
        max_grad_norm = _cfg(config, "TRAIN.CLIP_GRAD", 5.0)
    clip = None if max_grad_norm is None or not max_grad_norm > 0 else float(max_grad_norm)
    O = _cfg(config, "OPTIMIZER", None)
    base_lr = float(_cfg(config, "LR_SCHEDULER.BASE_LR", 1e-4))
    eps, betas = float(_cfg(O, "EPS", 1e-8)), tuple(_cfg(O, "BETAS", (0.9, 0.999, 0.9999)))
    momentum, wd_default = float(_cfg(O, "MOMENTUM", 0.9)), float(_cfg(O, "WEIGHT_DECAY", 0.05))
    alpha, t_ab3 = float(_cfg(O, "ALPHA", 5.0)), _cfg(O, "T_ALPHA_BETA3", None)
    muon_kw = dict(momentum=float(_cfg(O, "MUON.MOMENTUM", 0.95)), nesterov=bool(_cfg(O, "MUON.NESTEROV", True)), ns_steps=int(_cfg(O, "MUON.NS_STEPS", 5)),
                   strict=bool(_cfg(O, "MUON.STRICT", False)))  # MUON.USE_DISTRIBUTED: FusedMuon all the same (sharding is out of scope)

    def make(kind, params, lr, wd, own_clip=None):
        if kind == "sgd":
            return FusedSGD(params, lr=lr, momentum=momentum, weight_decay=wd, nesterov=True, max_grad_norm=own_clip)
        if kind == "adamw":
            return FusedAdamW(params, lr=lr, eps=eps, betas=betas[:2], weight_decay=wd, max_grad_norm=own_clip)
        if kind == "ademamix":
            return FusedAdEMAMix(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, alpha=alpha, T_alpha_beta3=t_ab3, max_grad_norm=own_clip)
        if kind == "muon":
            return FusedMuon(params, lr=lr, weight_decay=wd, max_grad_norm=own_clip, **muon_kw)
        raise ValueError(f"Unknown optimizer: {kind}")

    def muon_split(params):
        """(matrices for Muon, the rest): 2-D first, then 4-D, as the reference concatenates them"""
        two, four = [p for p in params if p.dim() == 2], [p for p in params if p.dim() == 4]
        return two + ([] if freeze_4d_like_reference else four), [p for p in params if p.dim() not in (2, 4)]

    if not bool(_cfg(O, "PARAMETER_GROUPS.ENABLED", False)):
        name = str(_cfg(O, "NAME", "adamw")).lower()
        if name in ("sgd", "adamw", "ademamix"):
            skip = model.no_weight_decay() if hasattr(model, "no_weight_decay") else ()
            skip_kw = model.no_weight_decay_keywords() if hasattr(model, "no_weight_decay_keywords") else ()
            return make(name, set_weight_decay(model, skip, skip_kw), base_lr, wd_default, clip)
        if name != "muon":
            raise ValueError(f"Unknown optimizer: {name}")
        cand, rest = [], []
        for n, p in model.named_parameters():
            if not p.requires_grad:
                continue
            (rest if any(k in n.lower() for k in MUON_SKIP_KEYWORDS) else cand).append(p)
        mats, other = muon_split(cand)
        adamw = other + rest
        if mats and adamw:
            return FusedMultiOptimizer({"MUON": make("muon", mats, base_lr, wd_default), "ADAMW": make("adamw", adamw, base_lr, wd_default)}, max_grad_norm=clip)
        if not mats and not adamw:
            raise ValueError("build_optimizer: the model has no trainable parameter")
        return make("muon", mats, base_lr, wd_default, clip) if mats else make("adamw", adamw, base_lr, wd_default, clip)  # one optimizer: bare

    G = _cfg(O, "PARAMETER_GROUPS", None)
    named = [(n, p) for n, p in model.named_parameters()]
    grouped, matched = {}, {}
    for gname, gcfg in G.items():
        if gname == "DEFAULT" or not isinstance(gcfg, dict) or "FILTER" not in gcfg:
            continue
        _check_filter_types(gcfg["FILTER"], gname)
        f = param_filter(gcfg["FILTER"])
        params = [p for n, p in named if f(n, p)]  # (the reference's filters see frozen parameters too)
        if not params:
            continue
        for n, p in named:
            if f(n, p):
                if id(p) in matched:
                    raise ValueError(f"build_optimizer: parameter '{n}' is matched by both parameter groups '{matched[id(p)]}' and '{gname}' (overlapping groups)")
                matched[id(p)] = gname
        grouped[gname] = params
    default_kind = str(_cfg(G, "DEFAULT.OPTIMIZER", "adamw")).lower()
    default_wd = float(_cfg(G, "DEFAULT.WEIGHT_DECAY", wd_default))
    unmatched = [p for n, p in named if p.requires_grad and id(p) not in matched]  # named_parameters() order (the reference: a set)
    optimizers = {}

    def add(gname, kind, params, lr, wd, muon_name, adamw_name):
        if kind == "muon":
            mats, other = muon_split(params)
            if mats:
                optimizers[muon_name] = make("muon", mats, lr, wd)
            if other:
                optimizers[adamw_name] = make("adamw", other, lr, wd)
        else:
            optimizers[gname] = make(kind, params, lr, wd)

    for gname, params in grouped.items():
        gcfg = G[gname]
        lr = base_lr * float(_cfg(gcfg, "LR_MULTIPLIER", 1.0))
        add(gname, str(_cfg(gcfg, "OPTIMIZER", default_kind)).lower(), params, lr, float(_cfg(gcfg, "WEIGHT_DECAY", default_wd)), gname, f"{gname}_ADAMW")
    if unmatched:
        if default_kind not in ("sgd", "adamw", "ademamix", "muon"):
            raise ValueError(f"Unknown optimizer: {default_kind}")
        add("DEFAULT", default_kind, unmatched, base_lr, default_wd, "DEFAULT_MUON", "DEFAULT_ADAMW")
    return FusedMultiOptimizer(optimizers, max_grad_norm=clip)
