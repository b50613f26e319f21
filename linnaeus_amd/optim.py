"""Optimizer + step glue on device: `FusedAdamW` is a `torch.optim.Optimizer` whose
`step()` is one HIP launch for the whole model, three with clipping -- the sum of squares of every gradient (per-workgroup
partials + a fixed-order fold: bit-identical on every data-parallel rank), then a multi-tensor AdamW update with the
global-norm clip folded in (csrc/optim.hip) -- instead of `clip_grad_norm_` (the reference makes three
gradient passes with host syncs, train.py:282-308) followed by `torch.optim.AdamW.step`.

Same update rule and `param_groups` / `state_dict` layout as `torch.optim.AdamW` (per-group `lr`, `betas`, `eps`,
`weight_decay`; per-parameter `step`, `exp_avg`, `exp_avg_sq`), so LR schedulers and the reference's parameter-group
builder (optimizers/build.py) work unchanged.  GPU fp32 parameters only.

`FusedAdEMAMix` is the same machinery for the reference's AdEMAMix (optimizers/ademamix.py): one launch per step over the
same descriptor table plus a parallel table of slow-EMA pointers, three with the clip.
"""
import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L


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


class FusedAdamW(torch.optim.Optimizer):
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
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        if clip:
            L.check(lib.lnx_grad_sumsq(C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self._sumsq.data_ptr()), C.c_void_p(self._sumsq_ws.data_ptr()), stream),
                    "lnx_grad_sumsq")
        L.check(lib.lnx_adamw_step(C.c_void_p(table.data_ptr()), n, blocks, C.byref(h), C.c_void_p(self._sumsq.data_ptr()) if clip else None,
                                   C.c_float(self.max_grad_norm if clip else 0.0), stream), "lnx_adamw_step")
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


class FusedAdEMAMix(torch.optim.Optimizer):
    """AdEMAMix (linnaeus/optimizers/ademamix.py, chosen by OPTIMIZER.NAME = ademamix in optimizers/build.py) as one
    multi-tensor HIP launch per step, three with clipping (lnx_grad_sumsq, then lnx_ademamix_step with the clip folded in),
    instead of the reference's ~13 tensor ops per parameter.

    Same constructor defaults, `param_groups` keys (lr, betas, eps, weight_decay, alpha, T_alpha_beta3) and per-parameter
    state (step, exp_avg, exp_avg_sq, exp_avg_slow) as the reference, so its checkpoints load with `load_state_dict` and
    the other way round, and LR schedulers and build.py's parameter groups work unchanged.  The update is the reference's,
    including its quirk of dividing the slow EMA by the first bias correction as well (csrc/optim.hip).

    `max_grad_norm` clips over THIS optimizer's parameters.  When linnaeus builds one optimizer per parameter group
    (PARAMETER_GROUPS.ENABLED), leave it None and clip once, over all parameters, before the steps.  GPU fp32 only.
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
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        if clip:
            L.check(lib.lnx_grad_sumsq(C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self._sumsq.data_ptr()), C.c_void_p(self._sumsq_ws.data_ptr()), stream),
                    "lnx_grad_sumsq")
        L.check(lib.lnx_ademamix_step(table.data_ptr(), table.data_ptr() + nbytes, n, blocks, C.byref(h), self._sumsq.data_ptr() if clip else None,
                                      self.max_grad_norm if clip else 0.0, stream), "lnx_ademamix_step")
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


class FusedMuon(torch.optim.Optimizer):
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
    Contiguous fp32 parameters and gradients on the GPU only.  Bit-reproducible: no atomics, the same inputs give the same
    parameters whatever else is in the optimizer, so data-parallel replicas that each run the whole step stay equal.
    """

    def __init__(self, params, lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5, strict=False):
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
        L.check(L.lib().lnx_muon_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_muon_step")
        return loss
