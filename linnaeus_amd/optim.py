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
`FusedMuon` the reference's Muon in a fixed number of launches, `ShardedFusedMuon` the same step with the matrices shared out over the
data-parallel ranks and the bf16 updates all-gathered (the reference's DistributedMuon), bit for bit.

`build_optimizer(config, model)` is the reference's optimizers/build.py with these classes, and `FusedMultiOptimizer` its
MultiOptimizer with the clip block of train.py:279-313 inside `step()`: one norm pass over every gradient of the run, the clip
coefficient applied by each sub-optimizer's kernel (`use_shared_clip`), nothing read back to the host.

All five take `nonfinite_guard=True`: the skipped step of `torch.amp.GradScaler` (train.py:279-312 steps through `scaler.step`),
decided on the device by the norm pass, and GradScaler's `found_inf` / `grad_scale` protocol (`_Clipped`).
"""
import ctypes as C
import math
from typing import Optional

import numpy as np
import torch

from . import _lib as L
from .loss import _cfg_get as _cfg, param_filter


def _closure_loss(closure):
    """the loss of an optimizer's closure, run with gradients enabled; None without a closure"""
    if closure is None:
        return None
    with torch.enable_grad():
        return closure()


def _dense_fp32(t, dev, shape=None):
    """a contiguous fp32 tensor on `dev` (and of `shape`): what the kernels index with flat offsets"""
    return t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and (shape is None or t.shape == shape)


def _desc_table(rows):
    """host lnx_adamw_desc table of [(slot, p, m, v)] (m, v: state tensors or None) and its total workgroup count"""
    blocks_of = L.lib().lnx_adamw_blocks
    arr = (L.AdamWDesc * len(rows))()
    blk = 0
    for d, (slot, p, m, v) in zip(arr, rows):  # slot: which entry of the hyper struct the kernel reads for this row
        d.p, d.m, d.v, d.g = p.data_ptr(), None if m is None else m.data_ptr(), None if v is None else v.data_ptr(), p.grad.data_ptr()
        d.n, d.group, d.block_start = p.numel(), slot, blk
        blk += blocks_of(C.c_int64(p.numel()))
    return arr, blk


def _upload(dev, *arrs):
    """ctypes tables, one behind the other, on the device in one copy: through pinned memory when there is a GPU, so the copy does
    not wait for the device"""
    host = torch.from_numpy(np.concatenate([np.frombuffer(a, dtype=np.uint8) for a in arrs]))
    if dev.type != "cuda":
        return host
    host = host.pin_memory()
    out = host.to(dev, non_blocking=True)
    out._lnx_host = host  # pinned source stays alive as long as the table
    return out


class _NormPass:
    """The global-norm pass: lnx_grad_sumsq over a device descriptor table (per-workgroup partials + a fixed-order fold) leaves the
    sum of squares of the table's gradients in `sumsq[0]` (a guarded pass, lnx_grad_sumsq_guarded, also the norm of the unscaled
    gradients in `sumsq[1]`).  An optimizer whose own table lists every gradient calls
    `run`; `over_grads` keeps a gradient-only table for the others, rebuilt only when a gradient pointer changes."""

    def __init__(self):
        self.sumsq = None      # the result: [sum of squares, norm of the unscaled gradients (written by a guarded pass only)] on the device
        self._partials = None  # one float per workgroup
        self._key = None       # what the table of over_grads was built for
        self._table = None     # (device table, rows, workgroups)

    def reserve(self, dev, blocks):
        if self.sumsq is None or self.sumsq.device != dev:
            self.sumsq = torch.zeros(2, device=dev, dtype=torch.float32)
        if self._partials is None or self._partials.device != dev or self._partials.numel() < blocks:
            self._partials = torch.empty(blocks, device=dev, dtype=torch.float32)

    def run(self, table, n, blocks, guard=None):
        """guard: the step's lnx_step_guard; the fold launch then also decides whether the step is skipped"""
        self.reserve(table.device, blocks)
        args = (C.c_void_p(table.data_ptr()), n, blocks, C.c_void_p(self.sumsq.data_ptr()), C.c_void_p(self._partials.data_ptr()))
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if guard is None:
            L.check(L.lib().lnx_grad_sumsq(*args, stream), "lnx_grad_sumsq")
        else:
            L.check(L.lib().lnx_grad_sumsq_guarded(*args, C.byref(guard), stream), "lnx_grad_sumsq_guarded")

    def over_grads(self, params, guard=None):
        key = tuple((p.grad.data_ptr(), p.numel()) for p in params)
        if key != self._key:
            arr, blocks = _desc_table([(0, p, None, None) for p in params])
            self._table = (_upload(params[0].grad.device, arr), len(params), blocks)
            self._key = key
        self.run(*self._table, guard)


class _Guard:
    """Device side of the non-finite guard: the flag of the last step (1: skipped) and the running count of skipped steps, and the
    lnx_step_guard of a step, which adds the `found_inf` / `grad_scale` tensors that `torch.amp.GradScaler.step` hangs on the
    optimizer for the duration of the call."""

    def __init__(self):
        self.flag = None     # fp32 [1]
        self.skipped = None  # int64 [1]

    def struct(self, dev, owner):
        if self.flag is None or self.flag.device != dev:
            self.flag = torch.zeros(1, device=dev, dtype=torch.float32)
            self.skipped = torch.zeros(1, device=dev, dtype=torch.int64)
        g = L.StepGuard()
        g.flag, g.skipped = self.flag.data_ptr(), self.skipped.data_ptr()
        for name in ("found_inf", "grad_scale"):
            t = getattr(owner, name, None)
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != 1 or t.device != dev:
                raise L.LnxError(f"{type(owner).__name__}: `{name}` must be a one-element fp32 tensor on the gradients' device (GradScaler on that device)")
            setattr(g, name, t.data_ptr())
        return g


class _Clipped:
    """What the fused optimizers and the multi-optimizer share: `max_grad_norm`, the norm pass and the norm it leaves, and the
    non-finite guard.

    `nonfinite_guard=True` is the skipped step of `torch.amp.GradScaler`, decided on the device: the norm pass runs at every step
    (also without a clip) and its fold launch raises a flag when the sum of squares is not finite -- an inf or NaN gradient, or a finite
    one whose square overflows fp32 (|g| above about 1.8e19) -- or when GradScaler's `found_inf` is non-zero.  Every kernel of the step
    reads the flag first and returns: parameters, state tensors, `.grad` and Muon's workspace stay as they were.  The host never learns
    of a skip, so `state["step"]` counts ATTEMPTED steps (torch leaves it alone on a skipped step), and a momentum buffer that FusedSGD
    creates on a skipped step starts at zero (the next step then forms (1 - dampening) g where torch clones g).  The optimizer then
    speaks GradScaler's protocol (`_step_supports_amp_scaling`): `scaler.step(opt)` hands it `found_inf` and, unless `scaler.unscale_(opt)`
    ran, `grad_scale`, which the kernels divide out as they read the gradients; no value is read back to the host."""

    max_grad_norm = None
    nonfinite_guard = False
    _guard = None

    def _init_guard(self, nonfinite_guard):
        self.nonfinite_guard = bool(nonfinite_guard)
        self._guard = _Guard() if self.nonfinite_guard else None

    @property
    def _step_supports_amp_scaling(self) -> bool:
        """what torch.amp.GradScaler.step looks for: true exactly when the guard is on (an unguarded optimizer takes torch's generic path)"""
        return self.nonfinite_guard

    def grad_norm(self) -> Optional[torch.Tensor]:
        """total (pre-clip) L2 norm of the gradients seen by the last clipped or guarded step (device scalar, no sync), with GradScaler's
        scale divided out; inf or NaN on a skipped step.  None without a clip and without the guard."""
        if self._norm.sumsq is None or (self.max_grad_norm is None and not self.nonfinite_guard):
            return None
        return self._norm.sumsq[1] if self.nonfinite_guard else self._norm.sumsq.sqrt()[0]

    def skipped_steps(self) -> Optional[torch.Tensor]:
        """how many steps the guard has skipped (device int64 scalar, no sync); None without the guard or before the first step"""
        return None if self._guard is None or self._guard.skipped is None else self._guard.skipped[0]

    def last_step_skipped(self) -> Optional[torch.Tensor]:
        """whether the guard skipped the last step (device bool scalar, no sync); None without the guard or before the first step"""
        return None if self._guard is None or self._guard.flag is None else self._guard.flag[0] != 0


class _SharedClip(_Clipped):
    """What the four fused optimizers share: `use_shared_clip(sumsq, max_norm)` hands the optimizer a device scalar with the sum of
    squares of ALL gradients of the run (FusedMultiOptimizer computes it once per step).  The optimizer then makes no norm pass of
    its own and its kernel clips by that scalar; `use_shared_clip(None)` restores its own behaviour.  `guard` is the lnx_step_guard of the pass that
    wrote the scalar (FusedMultiOptimizer's union pass, which decides for every sub-optimizer): the kernels then obey its flag and divide
    its `grad_scale` out, and `max_norm` may be None (a guarded run without a clip)."""

    _shared = None

    def use_shared_clip(self, sumsq: Optional[torch.Tensor], max_norm: Optional[float] = None, guard=None):
        if sumsq is None:
            self._shared = None
            return
        if getattr(self, "max_grad_norm", None) is not None:
            raise ValueError(f"{type(self).__name__}: max_grad_norm is set; an optimizer clips either by its own norm or by a shared one")
        if not isinstance(sumsq, torch.Tensor) or sumsq.dtype != torch.float32 or sumsq.numel() != 1:
            raise ValueError("use_shared_clip: sumsq must be a one-element fp32 tensor")
        if guard is not None and self.nonfinite_guard:
            raise ValueError(f"{type(self).__name__}: nonfinite_guard is set; a step is guarded either by the optimizer's own norm pass or by a shared one")
        if (max_norm is None and guard is None) or (max_norm is not None and not max_norm > 0):
            raise ValueError(f"use_shared_clip: max_norm must be positive, got {max_norm}")
        self._shared = (sumsq, 0.0 if max_norm is None else float(max_norm), guard)

    def _clip(self, dev, norm_pass):
        """(pointer of the sum of squares or None, max_norm, lnx_step_guard or None) of this step; norm_pass(guard) is run when the
        optimizer clips or guards by itself"""
        if self._shared is not None:
            return self._shared[0].data_ptr(), self._shared[1], self._shared[2]
        clip = self.max_grad_norm is not None and self.max_grad_norm > 0
        if clip or self.nonfinite_guard:
            guard = self._guard.struct(dev, self) if self.nonfinite_guard else None
            norm_pass(guard)
            return self._norm.sumsq.data_ptr(), float(self.max_grad_norm) if clip else 0.0, guard
        return None, 0.0, None


class _ElementwiseOptimizer(_SharedClip, torch.optim.Optimizer):
    """The step of FusedAdamW, FusedAdEMAMix and FusedSGD: every parameter with a gradient becomes one row of a device descriptor
    table, every distinct (parameter group, `_state`'s slot key) pair one slot of the hyper struct, and the update is one launch over
    the table -- after a norm pass over the same table when the optimizer clips by itself.  The table is rebuilt, and the state
    tensors are validated, only when a slot or a pointer changed.  A subclass gives
      _STATE, _SLOT, _Hyper                    its state keys (the first two are desc.m and desc.v), what its slot key is, its hyper struct
      _state(group, p)                         (slot key, state tensors in _STATE order) of p for this step, the state created on first use
      _fill(h, si, group, slot_key)            slot si of the hyper struct
      _launch(table, n, blocks, h, sumsq, max_norm, guard, stream)    its lnx_*_step over the table (device address, rows, workgroups),
                                               the _guarded entry point when the step carries an lnx_step_guard
    and may give `_check_group` and `_behind`."""

    def _init_step(self, max_grad_norm, nonfinite_guard=False):
        self.max_grad_norm = max_grad_norm
        self._init_guard(nonfinite_guard)
        self._table = None  # (device table, rows, workgroups)
        self._key = None    # slot and pointers of every row of the table
        self._norm = _NormPass()

    @staticmethod
    def _check_group(group):
        """validation of a group that is repeated at every step: a loaded state dict or a scheduler may have changed it"""

    def _behind(self, items):
        """further ctypes tables that go behind the descriptors in the same upload"""
        return ()

    def _build(self, items):
        dev = items[0][1].device
        for _, p, tensors in items:  # the kernel indexes every state tensor with the parameter's offsets
            for k, t in zip(self._STATE, tensors):
                if not _dense_fp32(t, dev, p.shape):
                    raise L.LnxError(f"{type(self).__name__}: state '{k}' must be a contiguous fp32 tensor of the parameter's shape on its device")
        arr, blocks = _desc_table([(si, p, *(tuple(tensors) + (None, None))[:2]) for si, p, tensors in items])
        self._table = (_upload(dev, arr, *self._behind(items)), len(items), blocks)
        self._norm.reserve(dev, blocks)

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        name = type(self).__name__
        slots, items, key = {}, [], []
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or g.dtype != torch.float32 or not g.is_contiguous():
                    raise L.LnxError(f"{name} needs contiguous fp32 parameters and gradients on the GPU")
                slot_key, tensors = self._state(group, p)
                si = slots.setdefault((gi, slot_key), len(slots))
                items.append((si, p, tensors))
                key.append((si, p.data_ptr(), g.data_ptr(), *[t.data_ptr() for t in tensors]))
        if not items:
            return loss
        if len(slots) > L.ADAMW_MAX_GROUPS:
            raise L.LnxError(f"{name}: {len(slots)} distinct (parameter group, {self._SLOT}) combinations, at most {L.ADAMW_MAX_GROUPS} are supported")
        if key != self._key:
            self._build(items)
            self._key = key
        h = self._Hyper()
        h.ngroups = len(slots)
        for (gi, slot_key), si in slots.items():
            self._fill(h, si, self.param_groups[gi], slot_key)
        table, n, blocks = self._table
        sumsq, max_norm, guard = self._clip(table.device, lambda guard: self._norm.run(table, n, blocks, guard))
        self._launch(table.data_ptr(), n, blocks, h, sumsq, max_norm, guard, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return loss


class _AdamFamily(_ElementwiseOptimizer):
    """State and hyper-parameters that AdamW and AdEMAMix share.  torch.optim.AdamW bias-corrects PER PARAMETER (its own step count).
    Parameters of one group normally share a step count, but one that was frozen for a while, had no gradient on some steps or came
    from a checkpoint with mixed steps does not: every distinct (group, step) pair gets its own hyper-parameter slot."""

    _SLOT = "step count"

    def _state(self, group, p):
        st = self.state[p]
        if len(st) == 0:
            st["step"] = 0
            for k in self._STATE:
                st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
        t = st["step"] = int(st["step"]) + 1  # int() also accepts the tensor a torch.optim.AdamW state_dict carries
        return t, [st[k] for k in self._STATE]

    def _fill(self, h, si, group, t):
        b1, b2 = group["betas"][:2]
        h.lr[si], h.beta1[si], h.beta2[si], h.eps[si], h.weight_decay[si] = group["lr"], b1, b2, group["eps"], group["weight_decay"]
        h.bias_c1[si], h.bias_c2[si] = 1.0 - b1 ** float(t), 1.0 - b2 ** float(t)
        h.omb1[si], h.omb2[si] = 1.0 - b1, 1.0 - b2


class FusedAdamW(_AdamFamily):
    _STATE = ("exp_avg", "exp_avg_sq")
    _Hyper = L.AdamWHyper

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None,
                 nonfinite_guard: bool = False):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid AdamW hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > L.ADAMW_MAX_GROUPS:
            raise ValueError(f"at most {L.ADAMW_MAX_GROUPS} parameter groups")
        self._init_step(max_grad_norm, nonfinite_guard)

    def _launch(self, table, n, blocks, h, sumsq, max_norm, guard, stream):
        if guard is None:
            L.check(L.lib().lnx_adamw_step(C.c_void_p(table), n, blocks, C.byref(h), C.c_void_p(sumsq), C.c_float(max_norm), stream), "lnx_adamw_step")
        else:
            L.check(L.lib().lnx_adamw_step_guarded(table, n, blocks, C.byref(h), sumsq, max_norm, C.byref(guard), stream), "lnx_adamw_step_guarded")


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


class FusedAdEMAMix(_AdamFamily):
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

    _STATE = ("exp_avg", "exp_avg_sq", "exp_avg_slow")
    _Hyper = L.AdEMAMixHyper

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999, 0.9999), eps: float = 1e-8, weight_decay: float = 0, alpha: float = 5.0,
                 T_alpha_beta3: Optional[float] = None, max_grad_norm: Optional[float] = None, nonfinite_guard: bool = False):
        _check_ademamix_group(lr, betas, eps, weight_decay, T_alpha_beta3)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, alpha=alpha, T_alpha_beta3=T_alpha_beta3))
        for g in self.param_groups:  # groups may carry their own values
            _check_ademamix_group(g["lr"], g["betas"], g["eps"], g["weight_decay"], g["T_alpha_beta3"])
        if len(self.param_groups) > L.ADAMW_MAX_GROUPS:
            raise ValueError(f"at most {L.ADAMW_MAX_GROUPS} parameter groups")
        self._init_step(max_grad_norm, nonfinite_guard)

    def _fill(self, h, si, group, t):
        # bias corrections, alpha_t and beta3_t all follow each parameter's own step count (as in the reference)
        super()._fill(h, si, group, t)
        b1, _, b3 = group["betas"]
        alpha_t, beta3_t = ademamix_schedule(t, group["alpha"], b1, b3, group["T_alpha_beta3"])
        h.alpha_t[si], h.beta3_t[si], h.omb3[si] = alpha_t, beta3_t, 1.0 - beta3_t

    def _behind(self, items):
        return ((C.c_uint64 * len(items))(*(tensors[2].data_ptr() for _, _, tensors in items)),)  # the slow-EMA pointer of every row

    def _launch(self, table, n, blocks, h, sumsq, max_norm, guard, stream):
        slow = table + n * C.sizeof(L.AdamWDesc)
        if guard is None:
            L.check(L.lib().lnx_ademamix_step(table, slow, n, blocks, C.byref(h), sumsq, max_norm, stream), "lnx_ademamix_step")
        else:
            L.check(L.lib().lnx_ademamix_step_guarded(table, slow, n, blocks, C.byref(h), sumsq, max_norm, C.byref(guard), stream), "lnx_ademamix_step_guarded")


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

    def __init__(self, params, lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5, strict=False, max_grad_norm: Optional[float] = None,
                 nonfinite_guard: bool = False):
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
        self._norm = _NormPass()  # own clip: over a gradient-only descriptor table
        self._init_guard(nonfinite_guard)

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

    def _launch_order(self):
        """[(group index, p)] of every parameter by descending ns_steps (stable: ties keep the parameter order), and those with a gradient,
        validated; ([], []) when no parameter has a gradient: nothing to do this step"""
        order = [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        for g in self.param_groups:
            if int(g["ns_steps"]) != g["ns_steps"] or g["ns_steps"] < 0:
                raise ValueError(f"Invalid ns_steps value: {g['ns_steps']}")
        order.sort(key=lambda it: -int(self.param_groups[it[0]]["ns_steps"]))
        with_grad = [p for _, p in order if p.grad is not None]
        if not with_grad:
            return [], []
        dev = with_grad[0].device
        for p in with_grad:  # a parameter without a gradient is not touched this step
            if not (p.is_cuda and _dense_fp32(p, dev)):
                raise L.LnxError("FusedMuon needs contiguous fp32 parameters on one GPU")
            if not _dense_fp32(p.grad, dev, p.shape):
                raise L.LnxError("FusedMuon needs contiguous fp32 gradients on the parameters' GPU")
        return order, with_grad

    def _order_key(self, order):
        return tuple((id(p), tuple(p.shape), int(self.param_groups[gi]["ns_steps"])) for gi, p in order)

    def _step_scalars(self, gi, p):
        """(decay, step) of lnx_muon_mat for parameter p of group gi: double on the host, rounded once by the struct"""
        g = self.param_groups[gi]
        rows, cols = _muon_shape(p)
        lr = float(g["lr"])
        return 1 - lr * float(g["weight_decay"]), lr * max(1, rows / cols) ** 0.5

    def _step_args(self, order, dev):
        """lnx_muon_step_args (without the clip and the guard) over `order`, matrices by descending ns_steps: the layout rebuilt when a
        shape or ns_steps changed, the table refilled and copied to the device when its bytes changed, momentum buffers created on first use"""
        key = self._order_key(order)
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
                if not _dense_fp32(buf, dev, p.shape):
                    raise L.LnxError("FusedMuon: state 'momentum_buffer' must be a contiguous fp32 tensor of the parameter's shape on its device")
                m.g, m.buf = p.grad.data_ptr(), buf.data_ptr()
            mom = float(g["momentum"])
            m.ns_steps, m.nesterov = int(g["ns_steps"]), 1 if g["nesterov"] else 0
            m.momentum, m.omm = mom, 1 - mom
            m.decay, m.step = self._step_scalars(gi, p)
        table, tiles, ws, part, info = self._dev
        raw = bytes(mats)
        if raw != self._sent:  # gradient pointers and learning rates usually move between steps; the layout does not
            table.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            self._sent = raw
        a = L.MuonStepArgs()
        a.n, a.mats, a.mats_dev, a.tiles_dev = len(order), C.addressof(mats), table.data_ptr(), tiles.data_ptr()
        a.workspace, a.workspace_bytes, a.partials = ws.data_ptr(), ws.numel(), part.data_ptr()
        return a

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        order, with_grad = self._launch_order()
        if not with_grad:
            return loss
        dev = with_grad[0].device
        a = self._step_args(order, dev)
        a.sumsq, a.max_norm, guard = self._clip(dev, lambda guard: self._norm.over_grads(with_grad, guard))
        if guard is not None:  # every launch of the step obeys its flag: the workspace's zero padding survives a skipped step
            a.guard = C.pointer(guard)
        L.check(L.lib().lnx_muon_step(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_muon_step")
        return loss


def muon_partition(shapes, ns_steps, world):
    """lnx_muon_partition (host only, no GPU) of n logical [rows, cols] shapes with their ns_steps over `world` ranks: (owner per matrix,
    offset per matrix in bf16 elements inside its owner's segment, seg_elems, cost per rank).  Longest-processing-time greedy over the
    MFMA FLOPs of the Newton-Schulz products; a pure function of its inputs, so every rank computes the same table."""
    n = len(shapes)
    flat = (C.c_int * (2 * max(n, 1)))(*(int(v) for s in shapes for v in s))
    ns = (C.c_int * max(n, 1))(*(int(v) for v in ns_steps))
    owner, off = (C.c_int * max(n, 1))(), (C.c_int64 * max(n, 1))()
    cost, seg = (C.c_int64 * max(int(world), 1))(), C.c_int64()
    L.check(L.lib().lnx_muon_partition(flat, ns, n, int(world), owner, off, C.byref(seg), cost), "lnx_muon_partition")
    return list(owner[:n]), list(off[:n]), int(seg.value), list(cost[:int(world)])


class _Done:
    """the work handle of a collective that has nothing to wait for"""

    def wait(self):
        return True


class ShardedFusedMuon(FusedMuon):
    """`FusedMuon` with the step split over data-parallel ranks (the reference's DistributedMuon, muon.py:200-428): every rank holds the same
    all-reduced gradients, runs momentum and Newton-Schulz only for the matrices it owns, and the ranks all-gather the bf16 updates.
    Each matrix gives the same bits alone or in a set, so the parameters are those of `FusedMuon`, bit for bit, on every rank.

      begin_step()   the owned table (`muon_partition` over the shapes and ns_steps of ALL parameters of ALL groups, with or without a
                     gradient, by descending ns_steps), lnx_muon_orthogonalize into this rank's segment of a persistent
                     [world * seg_elems] bf16 buffer (3 * max(ns_steps) + 3 launches; none on a rank that owns nothing), then the gather
      finish_step()  waits for the gather; lnx_muon_apply_packed updates ALL matrices from the gathered buffer in one launch
      step()         both in turn.  `FusedMultiOptimizer.step` puts the other sub-optimizers' launches between the two.

    process_group / rank / world_size: rank and world size default to the process group's (the default group when None).
    gather(out, seg): a seam that replaces the collective (tests, the benchmark): `seg` is this rank's part of `out`, a view into it; it
    returns a work handle (`.wait()`) or None.  The default is `dist.all_gather_into_tensor(out, seg, group, async_op=True)`, or
    `dist.all_gather` over `world` views of `out` where the backend refuses that call; at world size 1 nothing is gathered.

    `max_grad_norm`, `use_shared_clip` and `nonfinite_guard` work as on `FusedMuon`: the norm pass runs over the gradients of ALL
    parameters, in FusedMuon's order, so every rank forms the same coefficient and the same flag.
    `momentum_buffer` exists only for owned parameters: `state_dict()` is the local shard, `full_state_dict()` a collective that
    returns what `FusedMuon.state_dict()` would, and `load_state_dict` takes either and keeps the owned part.  The bf16 workspace
    and the fp32 momentum are this rank's share."""

    def __init__(self, params, lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5, strict=False, max_grad_norm: Optional[float] = None,
                 nonfinite_guard: bool = False, process_group=None, rank=None, world_size=None, gather=None):
        super().__init__(params, lr=lr, weight_decay=weight_decay, momentum=momentum, nesterov=nesterov, ns_steps=ns_steps, strict=strict,
                         max_grad_norm=max_grad_norm, nonfinite_guard=nonfinite_guard)
        if rank is None or world_size is None:
            import torch.distributed as dist

            if not (dist.is_available() and dist.is_initialized()):
                raise ValueError("ShardedFusedMuon: torch.distributed is not initialised; give rank and world_size (and a gather seam) or a process group")
            rank = dist.get_rank(process_group) if rank is None else rank
            world_size = dist.get_world_size(process_group) if world_size is None else world_size
        if int(world_size) < 1 or not 0 <= int(rank) < int(world_size):
            raise ValueError(f"ShardedFusedMuon: rank {rank} of world size {world_size}")
        self.process_group, self.rank, self.world_size, self._gather_seam = process_group, int(rank), int(world_size), gather
        self._part_key = None  # what the partition was computed for
        self._part = None      # (owner, elem_off, seg_elems, cost) in launch order
        self._gathered = None  # bf16 [world * seg_elems]: the ranks' segments, persistent
        self._out_off = None   # (host int64 array, device tensor) of the owned matrices' offsets in this rank's segment
        self._packed = None    # (host lnx_muon_packed table, device copy, bytes last sent)
        self._pending = None   # between begin_step and finish_step: (launch order, device, guard, work handle)
        self.collective = None  # which torch.distributed call the last default gather made

    # ------------------------------------------------------------------ partition
    def _all_order(self):
        order = [(gi, p) for gi, g in enumerate(self.param_groups) for p in g["params"]]
        order.sort(key=lambda it: -int(self.param_groups[it[0]]["ns_steps"]))
        return order

    def _partition(self, order=None):
        order = self._all_order() if order is None else order
        key = self._order_key(order)
        if key != self._part_key:
            self._part = muon_partition([_muon_shape(p) for _, p in order], [int(self.param_groups[gi]["ns_steps"]) for gi, _ in order], self.world_size)
            self._part_key = key
            self._gathered = self._out_off = self._packed = None
        return self._part

    def owns(self, p) -> bool:
        order = self._all_order()
        owner = self._partition(order)[0]
        return any(q is p and owner[i] == self.rank for i, (_, q) in enumerate(order))

    def partition_report(self) -> dict:
        """host only: owner of every parameter (param_groups order), cost per rank (Newton-Schulz MFMA FLOPs), their max / mean, seg_elems, and
        the bytes of this rank's workspace and of the gathered buffer"""
        order = self._all_order()
        owner, _, seg, cost = self._partition(order)
        by_id = {id(p): owner[i] for i, (_, p) in enumerate(order)}
        mine = [_muon_shape(p) for i, (_, p) in enumerate(order) if owner[i] == self.rank]
        mean = sum(cost) / len(cost)
        return {"rank": self.rank, "world_size": self.world_size, "owner": [by_id[id(p)] for g in self.param_groups for p in g["params"]], "cost": cost,
                "max_over_mean": max(cost) / mean if mean > 0 else 1.0, "seg_elems": seg,
                "workspace_bytes": int(muon_layout(mine)[2].workspace_bytes) if mine else 0, "gathered_bytes": 2 * seg * self.world_size}

    # ------------------------------------------------------------------ step
    def _gather(self, out, seg):
        if self._gather_seam is not None:
            return self._gather_seam(out, seg)
        if self.world_size == 1:
            return None  # the segment is the buffer
        import torch.distributed as dist

        try:
            work = dist.all_gather_into_tensor(out, seg, group=self.process_group, async_op=True)
            self.collective = "all_gather_into_tensor"
        except (RuntimeError, NotImplementedError):  # a backend without that call for these tensors: the list form over views of `out`
            work = dist.all_gather(list(out.view(self.world_size, -1).unbind(0)), seg, group=self.process_group, async_op=True)
            self.collective = "all_gather"
        return work

    @torch.no_grad()
    def begin_step(self):
        if self._pending is not None:
            raise L.LnxError("ShardedFusedMuon: begin_step twice without finish_step")
        order, with_grad = self._launch_order()
        if not with_grad:
            return
        dev = with_grad[0].device
        owner, elem_off, seg_elems, _ = self._partition(order)
        if self._gathered is None or self._gathered.device != dev:
            self._gathered = torch.zeros(self.world_size * seg_elems, device=dev, dtype=torch.bfloat16)
        mine = [i for i in range(len(order)) if owner[i] == self.rank]
        sumsq, max_norm, guard = self._clip(dev, lambda guard: self._norm.over_grads(with_grad, guard))  # over ALL gradients: the same on every rank
        seg = self._gathered[self.rank * seg_elems:(self.rank + 1) * seg_elems]
        if mine:
            a = self._step_args([order[i] for i in mine], dev)
            a.sumsq, a.max_norm = sumsq, max_norm
            if guard is not None:
                a.guard = C.pointer(guard)
            off = np.asarray([elem_off[i] for i in mine], dtype=np.int64)
            if self._out_off is None or not np.array_equal(self._out_off[0], off) or self._out_off[1].device != dev:
                self._out_off = (off, torch.from_numpy(off).to(dev))
            L.check(L.lib().lnx_muon_orthogonalize(C.byref(a), C.c_void_p(self._out_off[0].ctypes.data), C.c_void_p(self._out_off[1].data_ptr()),
                                                   C.c_void_p(seg.data_ptr()), seg_elems, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                    "lnx_muon_orthogonalize")
        self._pending = (order, dev, guard, self._gather(self._gathered, seg))

    @torch.no_grad()
    def finish_step(self):
        if self._pending is None:
            return  # begin_step found no gradient
        order, dev, guard, work = self._pending
        self._pending = None
        if work is not None:
            work.wait()
        owner, elem_off, seg_elems, _ = self._part
        n = len(order)
        if self._packed is None or len(self._packed[0]) != n or self._packed[1].device != dev:
            table = (L.MuonPacked * n)()
            self._packed = [table, torch.empty(C.sizeof(table), device=dev, dtype=torch.uint8), None]
        table = self._packed[0]
        blk = 0
        for i, (gi, p) in enumerate(order):
            d = table[i]
            d.p, d.numel, d.block_start = p.data_ptr(), p.numel(), blk
            d.off = -1 if p.grad is None else owner[i] * seg_elems + elem_off[i]
            d.decay, d.step = self._step_scalars(gi, p)
            blk += -(-p.numel() // L.MUON_ELEMS)
        raw = bytes(table)
        if raw != self._packed[2]:
            self._packed[1].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            self._packed[2] = raw
        L.check(L.lib().lnx_muon_apply_packed(C.addressof(table), C.c_void_p(self._packed[1].data_ptr()), n, C.c_void_p(self._gathered.data_ptr()), seg_elems,
                                              self.world_size, None if guard is None else C.pointer(guard), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                "lnx_muon_apply_packed")

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        self.begin_step()
        self.finish_step()
        return loss

    # ------------------------------------------------------------------ state
    def _state_segment(self):
        """this rank's part of the buffer `full_state_dict` gathers, fp32 [n + seg_elems]: one flag per matrix in launch order (1: owned here
        and holding a momentum buffer), then the owned momentum buffers at their segment offsets"""
        order = self._all_order()
        owner, elem_off, seg_elems, _ = self._partition(order)
        dev = next((self.state[p]["momentum_buffer"].device for _, p in order if "momentum_buffer" in self.state.get(p, {})), order[0][1].device)
        seg = torch.zeros(len(order) + seg_elems, device=dev, dtype=torch.float32)
        for i, (_, p) in enumerate(order):
            buf = self.state.get(p, {}).get("momentum_buffer") if owner[i] == self.rank else None
            if buf is not None:
                seg[i] = 1.0
                seg[len(order) + elem_off[i]:len(order) + elem_off[i] + p.numel()].copy_(buf.reshape(-1))
        return seg

    @torch.no_grad()
    def full_state_dict(self) -> dict:
        """A COLLECTIVE (every rank calls it): the state dict `FusedMuon` would write, with every momentum buffer, on every rank."""
        order = self._all_order()
        owner, elem_off, seg_elems, _ = self._partition(order)
        n, width = len(order), len(order) + seg_elems
        mine = self._state_segment()
        out = torch.empty(self.world_size * width, device=mine.device, dtype=torch.float32)
        seg = out[self.rank * width:(self.rank + 1) * width]
        seg.copy_(mine)
        work = self._gather(out, seg)
        if work is not None:
            work.wait()
        rows = out.view(self.world_size, width)
        flags = rows[:, :n].cpu()
        sd = super().state_dict()
        index = {id(p): k for k, p in enumerate(p for g in self.param_groups for p in g["params"])}  # torch packs the parameters 0, 1, ... in group order
        state = {}
        for i, (_, p) in enumerate(order):
            if flags[owner[i], i] != 0:
                lo = n + elem_off[i]
                state[index[id(p)]] = {"momentum_buffer": rows[owner[i], lo:lo + p.numel()].reshape(p.shape).clone()}
        sd["state"] = {k: state[k] for k in sorted(state)}
        return sd

    def load_state_dict(self, state_dict: dict) -> None:
        """takes the local shard or a full state dict (FusedMuon's, Muon's, the reference's) and keeps the owned part"""
        super().load_state_dict(state_dict)
        order = self._all_order()
        owner = self._partition(order)[0]
        for i, (_, p) in enumerate(order):
            if owner[i] != self.rank:
                self.state.pop(p, None)


# ----------------------------------------------------------------------------------------------------------------------
# SGD (OPTIMIZER.NAME = sgd; optimizers/build.py always builds it with nesterov=True): torch.optim.SGD's update as one launch
# ----------------------------------------------------------------------------------------------------------------------
class FusedSGD(_ElementwiseOptimizer):
    """`torch.optim.SGD` as one multi-tensor HIP launch per step (lnx_sgd_step), three with clipping, instead of torch's foreach
    passes.  Same `param_groups` keys and per-parameter state (`momentum_buffer`) as `torch.optim.SGD`, so state dicts load both
    ways; a missing or None buffer means "first step for this parameter" (the buffer then starts as the decayed gradient, as in
    torch).  One hyper-parameter slot per distinct (group, first step or not) pair.  `maximize=True` is refused, as is whatever
    torch's constructor refuses (Nesterov without momentum or with dampening, negative values).  A parameter without `.grad` is
    skipped.  `max_grad_norm` clips over THIS optimizer's parameters; `use_shared_clip` takes a run's norm instead.  GPU fp32 only.
    """

    _STATE = ("momentum_buffer",)
    _SLOT = "first step or not"
    _Hyper = L.SGDHyper

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0, dampening: float = 0, weight_decay: float = 0, nesterov: bool = False,
                 max_grad_norm: Optional[float] = None, nonfinite_guard: bool = False):
        # torch's own constructor checks and its group keys (maximize, foreach, differentiable, fused, ...), whatever the torch version
        defaults = dict(torch.optim.SGD([torch.zeros(1)], lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov).defaults)
        super().__init__(params, defaults)
        for g in self.param_groups:
            self._check_group(g)
        if len(self.param_groups) > L.ADAMW_MAX_GROUPS // 2:
            raise ValueError(f"at most {L.ADAMW_MAX_GROUPS // 2} parameter groups (two hyper-parameter slots each)")
        self._init_step(max_grad_norm, nonfinite_guard)

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

    def _state(self, group, p):
        if group["momentum"] == 0:
            return False, ()
        st = self.state[p]
        buf = st.get("momentum_buffer")
        first = buf is None
        if first:
            # the kernel writes all of it -- unless a guard skips the step: the buffer then has to read as "no momentum yet"
            guarded = self.nonfinite_guard or (self._shared is not None and self._shared[2] is not None)
            buf = st["momentum_buffer"] = (torch.zeros_like if guarded else torch.empty_like)(p, memory_format=torch.preserve_format)
        return first, (buf,)

    def _fill(self, h, si, g, first):
        h.lr[si], h.momentum[si], h.dampening[si], h.weight_decay[si] = g["lr"], g["momentum"], g["dampening"], g["weight_decay"]
        h.nesterov[si], h.first[si] = 1 if g["nesterov"] else 0, 1 if first else 0

    def _launch(self, table, n, blocks, h, sumsq, max_norm, guard, stream):
        if guard is None:
            L.check(L.lib().lnx_sgd_step(table, n, blocks, C.byref(h), sumsq, max_norm, stream), "lnx_sgd_step")
        else:
            L.check(L.lib().lnx_sgd_step_guarded(table, n, blocks, C.byref(h), sumsq, max_norm, C.byref(guard), stream), "lnx_sgd_step_guarded")


# ----------------------------------------------------------------------------------------------------------------------
# The configured optimizer (optimizers/build.py + optimizers/multi_optimizer.py + the clip block of train.py:279-313)
# ----------------------------------------------------------------------------------------------------------------------
FUSED_OPTIMIZERS = (FusedAdamW, FusedAdEMAMix, FusedSGD, FusedMuon)  # (ShardedFusedMuon is a FusedMuon)


class FusedMultiOptimizer(_Clipped):
    """The reference's `MultiOptimizer` (same interface: `optimizers`, `param_groups` carrying `optimizer_name` /
    `optimizer_group_idx`, `step`, `zero_grad`, `add_param_group`, `state_dict`, `load_state_dict`) with the gradient clip of
    train.py:279-313 inside `step()`: with `max_grad_norm`, ONE lnx_grad_sumsq pass (two launches, fixed-order fold) over every
    gradient of every sub-optimizer, then every sub-optimizer steps with that device scalar (`use_shared_clip`): its kernel
    scales the gradients as it reads them.  Nothing is read back to the host.

    The union table lists the parameters by SORTED optimizer name, then group, then position in the group -- the order of the
    stable state-dict indices -- so the norm's bits do not depend on the order the optimizers were inserted in.  It is rebuilt
    only when a gradient pointer changes.  `.grad` is left as it was (clip_grad_norm_ scales it in place).

    `nonfinite_guard=True` (see `_Clipped`): the union pass runs at every step, with or without a clip, and decides for all
    sub-optimizers at once; `scaler.step(multi)` works as on a single fused optimizer, the `found_inf` / `grad_scale` it sets here going
    to every sub-optimizer's kernels with the pass's flag.

    Refused: a sub-optimizer with its own `max_grad_norm` or `nonfinite_guard`; with a clip or the guard, a sub-optimizer that is not
    FusedAdamW, FusedAdEMAMix, FusedSGD or FusedMuon; a parameter held by two sub-optimizers (the reference would step it twice).

    `state_dict()` writes the layout the reference's code intends but does not produce (its saved per-optimizer "state" is always
    empty): `_version` 2, `_param_shapes`, `optimizers[name] = {"state": {stable index: ...}, "param_groups"}`.
    """

    def __init__(self, optimizers: dict, max_grad_norm: Optional[float] = None, nonfinite_guard: bool = False):
        self.optimizers = optimizers
        self.max_grad_norm = None if max_grad_norm is None or not max_grad_norm > 0 else float(max_grad_norm)
        self._init_guard(nonfinite_guard)
        seen = {}
        for name, opt in optimizers.items():
            if getattr(opt, "max_grad_norm", None) is not None:
                raise ValueError(f"FusedMultiOptimizer: sub-optimizer '{name}' has its own max_grad_norm; the clip is global, set it on the multi-optimizer")
            if getattr(opt, "nonfinite_guard", False):
                raise ValueError(f"FusedMultiOptimizer: sub-optimizer '{name}' has its own nonfinite_guard; one pass decides for all, set it on the multi-optimizer")
            if (self.max_grad_norm is not None or self.nonfinite_guard) and not isinstance(opt, FUSED_OPTIMIZERS):
                raise ValueError(f"FusedMultiOptimizer: sub-optimizer '{name}' ({type(opt).__name__}) is not a fused optimizer; "
                                 "the shared clip and the non-finite guard need FusedAdamW, FusedAdEMAMix, FusedSGD or FusedMuon")
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
        self._norm = _NormPass()  # over the union table

    # ------------------------------------------------------------------ step
    def _ordered_params(self):
        """every parameter in stable order: sorted optimizer name, group, position"""
        return [p for name in sorted(self.optimizers) for g in self.optimizers[name].param_groups for p in g["params"]]

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        if self.max_grad_norm is not None or self.nonfinite_guard:
            with_grad = [p for p in self._ordered_params() if p.grad is not None]
            if with_grad:
                dev = with_grad[0].device
                for p in with_grad:
                    if not (p.grad.is_cuda and _dense_fp32(p.grad, dev)):
                        raise L.LnxError("FusedMultiOptimizer needs contiguous fp32 gradients on one GPU")
                guard = self._guard.struct(dev, self) if self.nonfinite_guard else None  # with GradScaler's found_inf / grad_scale
                self._norm.over_grads(with_grad, guard)  # the union table
                for opt in self.optimizers.values():
                    opt.use_shared_clip(self._norm.sumsq[:1], self.max_grad_norm, guard)
        # a sharded sub-optimizer's gather runs under the other sub-optimizers' launches: begin (orthogonalise, issue the gather), the others, finish
        sharded = [opt for opt in self.optimizers.values() if isinstance(opt, ShardedFusedMuon)]
        for opt in sharded:
            opt.begin_step()
        for opt in self.optimizers.values():
            if not isinstance(opt, ShardedFusedMuon):
                opt.step()
        for opt in sharded:
            opt.finish_step()
        return loss

    def grad_norms(self):
        """(pre-clip norm, post-clip norm, the value clip_grad_norm_ returned) of the last step, the three values train.py:339-348
        logs, as device scalars.  The post-clip norm is pre * coef with the kernels' coef = min(1, max / (pre + 1e-6)); the reference
        measures the clipped gradients again.  The third equals the first."""
        pre = self.grad_norm()
        if pre is None:
            return None
        if self.max_grad_norm is None:  # guarded, not clipped
            return pre, pre, pre
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


def build_optimizer(config, model, max_grad_norm="config", freeze_4d_like_reference: bool = False, nonfinite_guard: bool = False):
    """optimizers/build.py's `build_optimizer`, branch for branch, with the fused classes: `OPTIMIZER.NAME` sgd / adamw / ademamix over
    the decay / no-decay split; muon as {"MUON": FusedMuon, "ADAMW": FusedAdamW}; and with `OPTIMIZER.PARAMETER_GROUPS.ENABLED` one
    optimizer per group (filters of `loss.param_filter`, `LR_MULTIPLIER`, `WEIGHT_DECAY`, `{group}_ADAMW` for the non-matrix parameters
    of a Muon group, `DEFAULT` / `DEFAULT_MUON` / `DEFAULT_ADAMW` for the unmatched ones, in named_parameters() order where the reference
    iterates a set).  Missing config nodes take the reference config.py's defaults.

    max_grad_norm: "config" reads TRAIN.CLIP_GRAD (default 5.0); None or <= 0: no clip.  A single optimizer gets it as its own
    `max_grad_norm`, several get it through `FusedMultiOptimizer`: either way the clip of train.py:279-313 is inside `step()`.
    4-D parameters selected for Muon are trained.  The reference never updates them (it hands Muon wrappers whose .grad stays None):
    freeze_4d_like_reference=True leaves them out of every optimizer, which is what the reference effectively does.
    nonfinite_guard: the device-side skipped step of GradScaler (see `_Clipped`), on the single optimizer or on the FusedMultiOptimizer.
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
                   strict=bool(_cfg(O, "MUON.STRICT", False)))
    # MUON.USE_DISTRIBUTED (the reference's DistributedMuon): the sharded step, but only where there is something to share the work with
    import torch.distributed as dist

    shard_muon = bool(_cfg(O, "MUON.USE_DISTRIBUTED", False)) and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

    def make(kind, params, lr, wd, own_clip=None, own_guard=False):
        own = dict(max_grad_norm=own_clip, nonfinite_guard=own_guard)
        if kind == "sgd":
            return FusedSGD(params, lr=lr, momentum=momentum, weight_decay=wd, nesterov=True, **own)
        if kind == "adamw":
            return FusedAdamW(params, lr=lr, eps=eps, betas=betas[:2], weight_decay=wd, **own)
        if kind == "ademamix":
            return FusedAdEMAMix(params, lr=lr, betas=betas, eps=eps, weight_decay=wd, alpha=alpha, T_alpha_beta3=t_ab3, **own)
        if kind == "muon":
            return (ShardedFusedMuon if shard_muon else FusedMuon)(params, lr=lr, weight_decay=wd, **own, **muon_kw)
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
            return make(name, set_weight_decay(model, skip, skip_kw), base_lr, wd_default, clip, nonfinite_guard)
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
            return FusedMultiOptimizer({"MUON": make("muon", mats, base_lr, wd_default), "ADAMW": make("adamw", adamw, base_lr, wd_default)}, max_grad_norm=clip,
                                       nonfinite_guard=nonfinite_guard)
        if not mats and not adamw:
            raise ValueError("build_optimizer: the model has no trainable parameter")
        return make("muon" if mats else "adamw", mats or adamw, base_lr, wd_default, clip, nonfinite_guard)  # one optimizer: bare

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
    return FusedMultiOptimizer(optimizers, max_grad_norm=clip, nonfinite_guard=nonfinite_guard)
