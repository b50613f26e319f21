"""Loss on device: the reference's soft-label criterion and the multi-task cross entropy
of the train step as single HIP launches (`lnx_softce`, csrc/loss.hip) behind the reference's module interface.

  TaxonomyAwareLabelSmoothingCE  <- linnaeus/loss/taxonomy_label_smoothing.py:131-408 (same constructor, same
                                    [B] per-sample return, same ignore_index / class-weight behaviour, same errors);
                                    from_tables / TaxonomySmoothingTables / generate_taxonomy_tables: the same criterion
                                    without the [C, C] matrix (<- utils/taxonomy/taxonomy_utils.py:24-254, taxonomy_tree.py:364-381)
  CrossEntropyLoss, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy
                                 <- linnaeus/loss/basic_loss.py:15-228, the other three names of LOSS.TASK_SPECIFIC.*.FUNCS
  get_loss_function / prepare_loss_functions <- linnaeus/loss/utils.py:58-294; convert_criteria maps criteria the reference
                                    built onto the classes here
  multitask_cross_entropy        <- the "per-task mean CE, static task weights, summed" loss of the throughput
                                    protocol; forward value and dlogits of all tasks without torch's
                                    log_softmax / nll_loss kernel chain

There is no CPU path: tensors must be on the GPU (LnxError otherwise), like the model itself.
"""
import ctypes as C
import math
import re
from typing import Any, Callable, Dict, Optional

import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib as L


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _fill(a, logits, target, soft, smoothing, class_weight, ignore_index, row_scale, scale, loss, loss_sum, dlogits, form=0, soft_target=None, sum_ws=None,
          tax=None):
    """`tax`: (anc, val, depth) of a criterion in table form (form CE_FORM_TAXONOMY), on the logits' device"""
    if not logits.is_cuda:
        raise L.LnxError("linnaeus_amd.loss has no CPU path: logits must be on the GPU")
    a.B, a.C = logits.shape
    a.logits, a.ld = _ptr(logits), logits.stride(0)
    a.target = _ptr(target)
    a.soft, a.smoothing = _ptr(soft), float(smoothing)
    a.class_weight = _ptr(class_weight)
    a.ignore_index = -1 if ignore_index is None else int(ignore_index)
    a.row_scale, a.scale = _ptr(row_scale), float(scale)
    a.loss, a.loss_sum = _ptr(loss), _ptr(loss_sum)
    a.dlogits, a.ldd = _ptr(dlogits), (dlogits.stride(0) if dlogits is not None else 0)
    a.form, a.soft_target, a.ldt = int(form), _ptr(soft_target), (soft_target.stride(0) if soft_target is not None else 0)
    a.sum_ws = _ptr(sum_ws)
    if tax is not None:
        a.tax_anc, a.tax_val, a.tax_depth = _ptr(tax[0]), _ptr(tax[1]), int(tax[2])


def _launch(*args):
    a = L.SoftCEArgs()
    _fill(a, *args)
    L.check(L.lib().lnx_softce(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_softce")


SOFTCE_MAX_TASKS = 8  # == LNX_SOFTCE_MAX_TASKS


def _launch_multi(sets):
    """`sets`: argument tuples of _fill, at most SOFTCE_MAX_TASKS per launch"""
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for i0 in range(0, len(sets), SOFTCE_MAX_TASKS):
        chunk = sets[i0:i0 + SOFTCE_MAX_TASKS]
        arr = (L.SoftCEArgs * len(chunk))()
        for a, args in zip(arr, chunk):
            _fill(a, *args)
        L.check(L.lib().lnx_softce_multi(arr, len(chunk), st), "lnx_softce_multi")


def _as_rows(logits):
    x = logits.float()
    return x if x.stride(-1) == 1 else x.contiguous()


class _SoftCE(torch.autograd.Function):
    """per-sample loss [B]; the unit gradient (d loss[b] / d logits[b, :]) is produced by the same launch"""

    @staticmethod
    def forward(ctx, logits, target, soft, class_weight, ignore_index, smoothing, form=0, soft_target=None, tax=None):
        x = _as_rows(logits)
        B, Cn = x.shape
        loss = torch.empty(B, device=x.device, dtype=torch.float32)
        need = logits.requires_grad
        unit = torch.empty(B, Cn, device=x.device, dtype=torch.float32) if need else None
        _launch(x, target, soft, smoothing, class_weight, ignore_index, None, 1.0, loss, None, unit, form, soft_target, None, tax)
        ctx.unit = unit
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, go):
        return (ctx.unit * go.unsqueeze(1)).to(ctx.in_dtype), None, None, None, None, None, None, None, None


class TaxonomyAwareLabelSmoothingCE(nn.Module):
    """Label-smoothing cross entropy whose soft labels come from a precomputed [C, C] distribution matrix
    (row c = distribution over classes when the true class is c).  Returns per-sample losses [B].

    `from_tables` builds the same criterion from TaxonomySmoothingTables instead: no [C, C] matrix exists anywhere, the kernel
    forms each row from the tables (`soft_labels` is None, the buffers are `tax_anc` / `tax_val`)."""

    def __init__(self, soft_label_matrix: torch.Tensor, weight: Optional[torch.Tensor] = None, apply_class_weights: bool = False,
                 ignore_index: Optional[int] = None, config: Optional[Any] = None):
        super().__init__()
        if soft_label_matrix.dim() != 2 or soft_label_matrix.shape[0] != soft_label_matrix.shape[1]:
            raise ValueError("soft_label_matrix must be square [C, C].")
        self.num_classes = soft_label_matrix.shape[0]
        self.register_buffer("soft_labels", soft_label_matrix.clone().float().contiguous())
        self.tables = None
        self._init_common(weight, apply_class_weights, ignore_index, config)

    def _init_common(self, weight, apply_class_weights, ignore_index, config):
        self.apply_class_weights = apply_class_weights
        self.ignore_index = ignore_index
        self.config = config
        self.validate_targets = True
        self.weight = None
        if weight is not None:
            if not isinstance(weight, torch.Tensor):
                weight = torch.tensor(weight, dtype=torch.float32)
            self.register_buffer("class_weight", weight.clone().float().contiguous())
            self.weight = self.class_weight

    @classmethod
    def from_tables(cls, tables: "TaxonomySmoothingTables", weight: Optional[torch.Tensor] = None, apply_class_weights: bool = False,
                    ignore_index: Optional[int] = None, config: Optional[Any] = None) -> "TaxonomyAwareLabelSmoothingCE":
        """The criterion of the matrix `tables` stand for, without the matrix: same forward, same `validate_targets` behaviour, same
        attributes, `soft_labels = None`, and the int32 [D, C] / fp32 [C, D + 2] buffers `tax_anc` / `tax_val` in its place."""
        if not isinstance(tables, TaxonomySmoothingTables):
            raise TypeError(f"from_tables needs TaxonomySmoothingTables, got {type(tables).__name__}")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.num_classes = tables.num_classes
        self.register_buffer("soft_labels", None)
        self.register_buffer("tax_anc", tables.anc.clone())
        self.register_buffer("tax_val", tables.val.clone())
        self.tables = tables
        self._init_common(weight, apply_class_weights, ignore_index, config)
        return self

    def _row_source(self, dev):
        """(soft, form, tax) for _fill on `dev`: the [C, C] matrix with the default form, or (anc, val, depth) with CE_FORM_TAXONOMY;
        the buffers are moved once when they live elsewhere"""
        if self.soft_labels is not None:
            if self.soft_labels.device != dev:
                self.soft_labels = self.soft_labels.to(dev)
            return self.soft_labels, L.CE_FORM_DEFAULT, None
        if self.tax_val.device != dev:
            self.tax_anc, self.tax_val = self.tax_anc.to(dev), self.tax_val.to(dev)
        return None, L.CE_FORM_TAXONOMY, (self.tax_anc, self.tax_val, self.tables.depth)

    def forward(self, logits, target: torch.Tensor) -> torch.Tensor:
        if isinstance(logits, dict):  # output of a ConditionalClassifierHead: first [B, num_classes] tensor
            found = None
            for value in logits.values():
                if isinstance(value, torch.Tensor) and value.ndim == 2 and value.shape[1] == self.num_classes:
                    found = value
                    break
            if found is None:
                shapes = {k: v.shape for k, v in logits.items() if isinstance(v, torch.Tensor)}
                raise ValueError(f"Could not find logits tensor with {self.num_classes} classes in input dict. Available shapes: {shapes}")
            logits = found
        elif not isinstance(logits, torch.Tensor):
            raise TypeError(f"Unsupported logits type: {type(logits)}. Expected Tensor or Dict.")
        if logits.shape[1] != self.num_classes:
            raise ValueError(f"Logits dimension mismatch. Expected {self.num_classes} classes, got {logits.shape[1]}.")
        if target.dim() == 2:
            target = target.argmax(dim=1)
        elif target.dim() != 1:
            raise ValueError(f"Target tensor has invalid shape {target.shape}. Expected 1D indices or [B, C] one-hot/soft-representing-one-class.")
        target = target.to(logits.device, torch.long).contiguous()
        soft, form, tax = self._row_source(logits.device)
        cw = None
        if self.apply_class_weights and self.weight is not None:
            if self.weight.device != logits.device:
                self.weight = self.class_weight = self.weight.to(logits.device)
            cw = self.weight
        loss = _SoftCE.apply(logits, target, soft, cw, self.ignore_index, 0.0, form, None, tax)
        # Out-of-range targets surface as NaN rows from the kernel; the reference raises IndexError for them
        # (taxonomy_label_smoothing.py:330-343, itself a host sync).  This check is ONE host<->device sync per call:
        # set `validate_targets = False` on the criterion to keep the launch queue asynchronous (NaN rows then
        # propagate into the loss instead of raising).
        if self.validate_targets and torch.isnan(loss).any():
            bad = ((target < 0) | (target >= self.num_classes)).sum().item()
            if bad:
                raise IndexError(f"{bad} target indices out of bounds [0, {self.num_classes - 1}].")
        return loss


# ----------------------------------------------------------------------------------------------------------------------
# The reference's other three criteria (loss/basic_loss.py), the default of LOSS.TASK_SPECIFIC.{TRAIN,VAL}.FUNCS among them.
# Same constructor arguments in the same order, same attributes, same [B] per-sample return; each forward is ONE lnx_softce
# launch that also leaves the unit gradient, as TaxonomyAwareLabelSmoothingCE above.
# Stated differences from the reference, common to the three:
#   * a target outside [0, C) (torch's -100 included: only `ignore_index` is ignored) gives a NaN loss and a zero gradient row;
#     with `validate_targets` (default True) the call then raises IndexError after ONE host read, set it to False to keep the
#     launch queue asynchronous;
#   * a `weight` whose length is not C raises ValueError at the first call (the reference indexes it and fails, or not, later).
# ----------------------------------------------------------------------------------------------------------------------
class _BasicCriterion(nn.Module):
    _form = L.CE_FORM_DEFAULT

    def _device_weight(self, dev, num_classes: int):
        """the [C] fp32 class weight on `dev`, uploaded once per (weight object, device); None when weights do not apply"""
        if self.weight is None or not self.apply_class_weights:
            return None
        w = self.weight
        cached = getattr(self, "_w_dev", None)
        if cached is None or cached[0] is not w or cached[1].device != dev:
            v = w if isinstance(w, torch.Tensor) else torch.tensor(w, dtype=torch.float32)
            cached = (w, v.detach().to(dev, torch.float32).contiguous())
            self._w_dev = cached
        if cached[1].dim() != 1 or cached[1].numel() != num_classes:
            raise ValueError(f"{type(self).__name__}: weight has {tuple(cached[1].shape)} entries, the logits have {num_classes} classes")
        return cached[1]

    @staticmethod
    def _class_indices(logits, target):
        if target.dim() == 2:
            if target.shape[1] != logits.size(1):
                raise ValueError(f"Target tensor shape {target.shape} incompatible with input shape {logits.shape}")
            target = target.argmax(dim=1)
        elif target.dim() != 1:
            raise ValueError(f"Target tensor has invalid shape {target.shape}. Expected 1D indices or [B, C] one-hot/soft-representing-one-class.")
        return target.to(logits.device, torch.long).contiguous()

    def _hard(self, logits, target, smoothing: float):
        if not isinstance(logits, torch.Tensor) or logits.dim() != 2:
            raise TypeError(f"{type(self).__name__}: logits must be a [B, C] tensor")
        target = self._class_indices(logits, target)
        num_classes = logits.shape[1]
        cw = self._device_weight(logits.device, num_classes)
        loss = _SoftCE.apply(logits, target, None, cw, self.ignore_index, smoothing, self._form, None)
        if self.validate_targets and torch.isnan(loss).any():  # ONE host read per call, as TaxonomyAwareLabelSmoothingCE
            bad = ((target < 0) | (target >= num_classes)).sum().item()
            if bad:
                raise IndexError(f"{bad} target indices out of bounds [0, {num_classes - 1}].")
        return loss


class CrossEntropyLoss(_BasicCriterion):
    """Per-sample cross entropy [B] (loss/basic_loss.py:15-92): `[B]` integer targets of any integer dtype, or `[B, C]` targets
    that are arg-maxed; rows whose class is `ignore_index` give loss 0 and gradient 0; `weight[class]` multiplies the loss only
    when `weight is not None and apply_class_weights`.  Differences from the reference: see the comment above this class."""

    def __init__(self, weight: Optional[torch.Tensor] = None, apply_class_weights: bool = False, ignore_index: Optional[int] = None):
        super().__init__()
        self.ignore_index = ignore_index
        self.criterion = nn.CrossEntropyLoss(weight=None, reduction="none", ignore_index=ignore_index if ignore_index is not None else -100)
        self.weight = weight
        self.apply_class_weights = apply_class_weights
        self.validate_targets = True

    def forward(self, input, target) -> torch.Tensor:
        return self._hard(input, target, 0.0)


class LabelSmoothingCrossEntropy(_BasicCriterion):
    """Per-sample label-smoothing cross entropy [B] (loss/basic_loss.py:95-185): `1 - smoothing` on the class and
    `smoothing / (C - 1)` on every other one (not torch's `smoothing / C` everywhere), targets, `ignore_index` and `weight` as
    CrossEntropyLoss.  C == 1 is refused by name (the reference divides by zero).  Other differences: see the comment above."""
    _form = L.CE_FORM_OFF_TARGET

    def __init__(self, weight: Optional[torch.Tensor] = None, smoothing: float = 0.1, apply_class_weights: bool = False,
                 ignore_index: Optional[int] = None, config: Optional[Any] = None):
        super().__init__()
        assert 0.0 <= smoothing < 1.0
        self.smoothing = smoothing
        self.confidence = 1.0 - smoothing
        self.weight = weight
        self.apply_class_weights = apply_class_weights
        self.ignore_index = ignore_index
        self.config = config
        self.validate_targets = True

    def forward(self, x, target) -> torch.Tensor:
        return self._hard(x, target, float(self.smoothing))


class SoftTargetCrossEntropy(_BasicCriterion):
    """Per-sample cross entropy against a `[B, C]` soft distribution (mixup / cutmix targets; loss/basic_loss.py:188-228):
    `-(target * log_softmax(x)).sum(1)`, times `<target, weight>` when `weight is not None and apply_class_weights`.  The row's
    sum is summed, not assumed to be 1 (gradient `softmax * sum(target) - target`).  There is no `ignore_index`.
    Differences from the reference: a `[B]` target raises ValueError (the reference broadcasts it against the logits); a row
    with NaN or infinite entries gives a NaN loss and a zero gradient row; a `weight` whose length is not C raises ValueError."""
    _form = L.CE_FORM_SOFT_ROW

    def __init__(self, weight: Optional[torch.Tensor] = None, apply_class_weights: bool = False):
        super().__init__()
        self.weight = weight
        self.apply_class_weights = apply_class_weights

    @staticmethod
    def _rows(logits, target):
        if target.dim() != 2 or target.shape != logits.shape:
            raise ValueError(f"SoftTargetCrossEntropy needs [B, C] targets of the logits' shape {tuple(logits.shape)}, got {tuple(target.shape)}")
        y = target.to(logits.device, torch.float32)
        return y if y.stride(1) == 1 else y.contiguous()

    def forward(self, x, target) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() != 2:
            raise TypeError("SoftTargetCrossEntropy: logits must be a [B, C] tensor")
        y = self._rows(x, target)
        cw = self._device_weight(x.device, x.shape[1])
        return _SoftCE.apply(x, None, None, cw, None, 0.0, self._form, y)


LOSS_FUNCTIONS = ("CrossEntropyLoss", "SoftTargetCrossEntropy", "LabelSmoothingCrossEntropy", "TaxonomyAwareLabelSmoothing")


def get_loss_function(loss_type: str, config, class_weights=None, is_train: bool = True, task_key: Optional[str] = None,
                      taxonomy_matrices: Optional[Dict[str, Any]] = None, ignore_index: Optional[int] = None, taxonomy_tree=None) -> nn.Module:
    """The criterion `loss_type` names (loss/utils.py:153-294: the same name table, the same LOSS.GRAD_WEIGHTING.CLASS.TRAIN / .VAL
    switch).  `taxonomy_matrices[task]` is a [C, C] tensor or TaxonomySmoothingTables (generate_taxonomy_tables: no matrix is built).  A class-weight dict {class: weight} becomes a [max index + 1] tensor with missing entries 1.0; a tensor is passed on.
    `taxonomy_tree` is accepted and unused, as in the reference."""
    apply_class_weights = config.LOSS.GRAD_WEIGHTING.CLASS.TRAIN if is_train else config.LOSS.GRAD_WEIGHTING.CLASS.VAL
    weight = None
    if apply_class_weights and isinstance(class_weights, dict) and class_weights:
        try:
            table = {int(k): float(v) for k, v in class_weights.items()}
            weight = torch.tensor([table.get(i, 1.0) for i in range(max(table) + 1)], dtype=torch.float32)
        except (ValueError, TypeError):
            weight = None
    elif isinstance(class_weights, torch.Tensor):
        weight = class_weights
    if loss_type == "CrossEntropyLoss":
        return CrossEntropyLoss(weight=weight, apply_class_weights=apply_class_weights, ignore_index=ignore_index)
    if loss_type == "SoftTargetCrossEntropy":
        return SoftTargetCrossEntropy(weight=weight, apply_class_weights=apply_class_weights)
    if loss_type == "LabelSmoothingCrossEntropy":
        smoothing = config.MODEL.LABEL_SMOOTHING if hasattr(config.MODEL, "LABEL_SMOOTHING") else 0.1
        return LabelSmoothingCrossEntropy(smoothing=smoothing, weight=weight, apply_class_weights=apply_class_weights, ignore_index=ignore_index,
                                          config=config)
    if loss_type == "TaxonomyAwareLabelSmoothing":
        if not task_key:
            raise ValueError("task_key must be provided for TaxonomyAwareLabelSmoothing")
        if taxonomy_matrices is None or task_key not in taxonomy_matrices:
            raise ValueError(f"No taxonomy smoothing matrix found for task '{task_key}'")
        if isinstance(taxonomy_matrices[task_key], TaxonomySmoothingTables):
            return TaxonomyAwareLabelSmoothingCE.from_tables(taxonomy_matrices[task_key], weight=weight, apply_class_weights=apply_class_weights,
                                                             ignore_index=ignore_index, config=config)
        return TaxonomyAwareLabelSmoothingCE(soft_label_matrix=taxonomy_matrices[task_key], weight=weight, apply_class_weights=apply_class_weights,
                                             ignore_index=ignore_index, config=config)
    raise ValueError(f"Unsupported loss function type: {loss_type}")


def _per_task(value, task_keys, name: str) -> list:
    if isinstance(value, (list, tuple)):
        if len(value) != len(task_keys):
            raise ValueError(f"{name} must match number of tasks. Expected {len(task_keys)}, got {len(value)}")
        return list(value)
    return [value for _ in task_keys]


def prepare_loss_functions(config, class_weights_train=None, class_weights_val=None, taxonomy_matrices: Optional[Dict[str, Any]] = None):
    """(criteria_train, criteria_val), {task: criterion} over config.DATA.TASK_KEYS_H5 from LOSS.TASK_SPECIFIC.TRAIN.FUNCS / VAL.FUNCS
    (loss/utils.py:58-150), with ignore_index = 0 under TRAIN.PHASE1_MASK_NULL_LOSS.  The class weights are {task: {class: weight}}
    (or tensors) per split: computing them from label counts (calculate_class_weights) stays with the caller."""
    task_keys = list(config.DATA.TASK_KEYS_H5)
    ignore_index = 0 if getattr(config.TRAIN, "PHASE1_MASK_NULL_LOSS", False) else None
    out = []
    for is_train, funcs, cws in ((True, config.LOSS.TASK_SPECIFIC.TRAIN.FUNCS, class_weights_train), (False, config.LOSS.TASK_SPECIFIC.VAL.FUNCS, class_weights_val)):
        funcs = _per_task(funcs, task_keys, "TRAIN.FUNCS" if is_train else "VAL.FUNCS")
        out.append({t: get_loss_function(f, config, (cws or {}).get(t), is_train, t, taxonomy_matrices, ignore_index) for f, t in zip(funcs, task_keys)})
    return out[0], out[1]


def convert_criterion(crit):
    """one criterion built by the reference -> the class here, recognised by its class name and read through its attributes"""
    if isinstance(crit, (_BasicCriterion, TaxonomyAwareLabelSmoothingCE)) or type(crit) is nn.CrossEntropyLoss:
        return crit
    name = type(crit).__name__
    try:
        if name == "CrossEntropyLoss":
            return CrossEntropyLoss(weight=crit.weight, apply_class_weights=crit.apply_class_weights, ignore_index=crit.ignore_index)
        if name == "LabelSmoothingCrossEntropy":
            return LabelSmoothingCrossEntropy(weight=crit.weight, smoothing=crit.smoothing, apply_class_weights=crit.apply_class_weights,
                                              ignore_index=crit.ignore_index, config=getattr(crit, "config", None))
        if name == "SoftTargetCrossEntropy":
            return SoftTargetCrossEntropy(weight=crit.weight, apply_class_weights=crit.apply_class_weights)
        if name == "TaxonomyAwareLabelSmoothingCE":
            if getattr(crit, "soft_labels", None) is None and isinstance(getattr(crit, "tables", None), TaxonomySmoothingTables):  # table form
                return TaxonomyAwareLabelSmoothingCE.from_tables(crit.tables, weight=crit.weight, apply_class_weights=crit.apply_class_weights,
                                                                 ignore_index=crit.ignore_index, config=getattr(crit, "config", None))
            return TaxonomyAwareLabelSmoothingCE(crit.soft_labels, weight=crit.weight, apply_class_weights=crit.apply_class_weights,
                                                 ignore_index=crit.ignore_index, config=getattr(crit, "config", None))
    except AttributeError as e:
        raise L.LnxError(f"convert_criteria: {name} lacks an attribute of the reference's class of that name: {e}") from None
    raise L.LnxError(f"convert_criteria: criterion {name} is not supported ({ACCEPTED_CRITERIA})")


def convert_criteria(criteria):
    """{task: criterion} built by the reference's own prepare_loss_functions -> the same dict over the classes here.  The classes of
    this module and torch.nn.CrossEntropyLoss instances are returned unchanged; anything else is refused by name (LnxError)."""
    if isinstance(criteria, dict):
        return {t: convert_criterion(c) for t, c in criteria.items()}
    return convert_criterion(criteria)


ACCEPTED_CRITERIA = ("TaxonomyAwareLabelSmoothingCE, CrossEntropyLoss, LabelSmoothingCrossEntropy, SoftTargetCrossEntropy "
                     "or torch.nn.CrossEntropyLoss(reduction='none')")


class _MultiCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, targets, smoothing, *logits):
        total = torch.zeros((), device=logits[0].device, dtype=torch.float32)
        xs = [_as_rows(lg) for lg in logits]
        # the gradients of all tasks live in one flat buffer: one launch fills them, one multiply scales them in backward
        sizes = [x.numel() if lg.requires_grad else 0 for x, lg in zip(xs, logits)]
        flat = torch.empty(sum(sizes), device=total.device, dtype=torch.float32) if any(sizes) else None
        grads, sets, off = [], [], 0
        det = L.is_deterministic()  # the rows' terms then reach `total` through a per-row buffer, folded in row order
        for w, t, x, n in zip(weights, targets, xs, sizes):
            d = flat[off:off + n].view_as(x) if n else None
            off += n
            rows = torch.empty(x.shape[0], device=total.device, dtype=torch.float32) if det else None
            sets.append((x, t, None, smoothing, None, None, None, w / x.shape[0], None, total, d, 0, None, rows))
            grads.append(d)
        _launch_multi(sets)
        ctx.flat, ctx.sizes = flat, sizes
        ctx.shapes = [x.shape for x in xs]
        ctx.dtypes = [lg.dtype for lg in logits]
        return total

    @staticmethod
    def backward(ctx, go):
        if ctx.flat is None:
            return (None, None, None) + (None,) * len(ctx.sizes)
        scaled = ctx.flat * go
        out, off = [], 0
        for n, shp, dt in zip(ctx.sizes, ctx.shapes, ctx.dtypes):
            out.append(scaled[off:off + n].view(shp).to(dt) if n else None)
            off += n
        return (None, None, None) + tuple(out)


def multitask_cross_entropy(outputs: Dict[str, torch.Tensor], targets: Dict[str, torch.Tensor], task_weights: Optional[Dict[str, float]] = None,
                            label_smoothing: float = 0.0) -> torch.Tensor:
    """sum over tasks of task_weight * mean over the batch of cross_entropy(outputs[task], targets[task]).
    One launch per task computes the loss contribution and d(loss)/d(logits); backward is a scalar multiply."""
    tasks = list(outputs.keys())
    ws = [1.0 if task_weights is None else float(task_weights[t]) for t in tasks]
    tg = [targets[t].to(outputs[t].device, torch.long).contiguous() for t in tasks]
    return _MultiCE.apply(ws, tg, float(label_smoothing), *[outputs[t] for t in tasks])


# ----------------------------------------------------------------------------------------------------------------------
# The whole loss path of the train step on device (remainder): weighted_hierarchical_loss with null
# masking, class weighting and static task weighting, plus the taxonomy smoothing-matrix builder.
#   build_taxonomy_smoothing_matrix <- loss/taxonomy_label_smoothing.py:30-130
#   compute_core_loss               <- loss/core_loss.py:19-100
#   apply_null_masking / apply_class_weighting / apply_loss_masking <- loss/masking.py:19-465, 469-518, 521-700
#   GradientWeighting               <- loss/gradient_weighting.py:178-880 (static and GradNorm), loss/gradnorm.py
#   weighted_hierarchical_loss      <- loss/hierarchical_loss.py:24-406
# The per-sample criterion runs in the HIP kernel (lnx_softce); everything after it is arithmetic on [B]-sized device
# vectors.  What changes against the reference is HOW, not WHAT: its per-sample Python loops with .item() (a host sync
# per sample, loss/masking.py:501-503, gradient_weighting.py:338-342) become one gather from a class-weight vector, and
# the valid-sample counts stay on the device.  Finding F13 is reproduced, not fixed: class weights enter three times on
# the scheduled-masking path, twice on the PHASE1 / validation paths, and the mean divides by count(loss != 0).
# ----------------------------------------------------------------------------------------------------------------------
def build_taxonomy_smoothing_matrix(num_classes: int, distances: torch.Tensor, alpha: float = 0.1, beta: float = 1.0,
                                    uniform_roots: bool = True, root_class_ids=None) -> torch.Tensor:
    """[C, C] soft-label matrix: row i = (1 - alpha) on the diagonal, alpha spread over the other classes in proportion
    to exp(-beta * distance) (uniformly for root classes, and for rows whose neighbours are all disconnected)."""
    if not (0.0 <= alpha <= 1.0):
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    if beta < 0:
        raise ValueError(f"beta must be non-negative, got {beta}")
    if num_classes <= 0:
        raise ValueError("num_classes must be positive.")
    if distances.shape != (num_classes, num_classes):
        raise ValueError(f"distances must be shape ({num_classes},{num_classes}), got {distances.shape}")
    C_ = num_classes
    d = distances.float()
    w = torch.exp(-beta * d)
    w = torch.where(torch.isinf(d), torch.zeros_like(w), w)
    eye = torch.eye(C_, dtype=torch.bool, device=d.device)
    w = w.masked_fill(eye, 0.0)
    if uniform_roots and root_class_ids and C_ > 1:
        roots = torch.as_tensor(list(root_class_ids), dtype=torch.long, device=d.device)
        w[roots] = torch.full((C_,), 1.0 / (C_ - 1), device=d.device)
        w = w.masked_fill(eye, 0.0)
    elif uniform_roots and root_class_ids and C_ == 1:
        w.zero_()
    rs = w.sum(1, keepdim=True)
    if C_ > 1:
        fallback = torch.full((C_, C_), alpha / (C_ - 1), device=d.device).masked_fill(eye, 0.0)
        probs = torch.where(rs > 1e-9, w * (alpha / rs.clamp_min(1e-30)), fallback)
    else:
        probs = torch.zeros_like(w)
    probs = probs.masked_fill(eye, 1.0 - alpha)
    tot = probs.sum(1, keepdim=True)
    return torch.where((tot - 1.0).abs() > 1e-6, probs / tot, probs)


# ----------------------------------------------------------------------------------------------------------------------
# Taxonomy smoothing without the [C, C] matrix.  Parents always sit at the next task level (utils/taxonomy/taxonomy_tree.py:
# 165-213), so two classes of one level are at distance 2k, k the first height at which their ancestor chains meet, or inf when
# they never meet.  Row i of build_taxonomy_smoothing_matrix(build_distance_matrix(...)) therefore holds at most D + 2 distinct
# values (D = levels above): 1 - alpha on the diagonal, one value per height, one for disconnected classes; and its normaliser
# follows from per-ancestor descendant counts in O(C * D).  The tables below hold exactly that: O(C * D) memory and build time
# instead of the reference's O(C^2) Python double loop, nothing to broadcast between ranks (each rank builds them locally).
#   n_k(i) = classes of the level sharing i's k-th ancestor (n_0 = 1; n_{k-1} where the chain has ended),  m_k = n_k - n_{k-1}
#   Z_i    = sum_k m_k(i) * exp(-2 beta k)
#   row i is UNIFORM (every off-diagonal entry alpha / (C - 1), disconnected classes included) when Z_i <= 1e-9, or when class i
#   has no parent and uniform_roots is set; otherwise val[i, k] = alpha * exp(-2 beta k) / Z_i and disconnected classes get 0.
# Everything is computed in fp64 and rounded to fp32 once.  Stated difference from the reference: it takes the Z <= 1e-9 decision
# on an fp32 sum of C terms, here it is taken on the fp64 closed form, so a row within rounding of the threshold can fall on the
# other side.  (The reference also divides a row by its fp32 sum when that is off 1 by more than 1e-6; the rows here sum to 1.)
# ----------------------------------------------------------------------------------------------------------------------
TAX_MAX_DEPTH = L.TAX_MAX_DEPTH


class TaxonomySmoothingTables:
    """The soft-label matrix of one task level as two small tables (host tensors; `to(device)` caches device copies):
      anc  int32 [D, C]   anc[k-1, c] = index at level + k of the k-th ancestor of class c, -1 once the chain has ended (level-major)
      val  fp32 [C, D+2]  val[i, 0] = 1 - alpha, val[i, k] = soft label true class i gives a class at distance 2k, val[i, D+1] =
                          soft label for a disconnected class
    `dense()` / `distances()` expand rows of the matrices they stand for on the GPU (lnx_taxonomy_rows)."""

    def __init__(self, anc: torch.Tensor, val: torch.Tensor, alpha: float, beta: float, val64=None, counts=None):
        self.anc, self.val = anc.to(torch.int32).contiguous(), val.to(torch.float32).contiguous()
        self.num_classes, self.depth = int(self.val.shape[0]), int(self.val.shape[1]) - 2
        if self.anc.shape != (self.depth, self.num_classes):
            raise ValueError(f"anc must be [{self.depth}, {self.num_classes}], got {tuple(self.anc.shape)}")
        self.alpha, self.beta = float(alpha), float(beta)
        self.val64, self.counts = val64, counts  # keep_fp64=True: the unrounded values and how many classes take each of them
        self._dev = {}

    @property
    def nbytes(self) -> int:
        return self.anc.numel() * 4 + self.val.numel() * 4

    @property
    def matrix_bytes(self) -> int:
        """what the fp32 [C, C] matrix these tables replace would take"""
        return 4 * self.num_classes * self.num_classes

    def to(self, device):
        """(anc, val) on `device`, uploaded once per device"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = (self.anc.to(device), self.val.to(device))
        return self._dev[device]

    def _rows(self, rows, device, what: int) -> torch.Tensor:
        anc, val = self.to(device or "cuda")
        dev = val.device
        if dev.type != "cuda":
            raise L.LnxError("TaxonomySmoothingTables.dense / distances run on the GPU (lnx_taxonomy_rows): there is no CPU path")
        if rows is not None:
            rows = torch.as_tensor(rows, dtype=torch.long).to(dev).contiguous().view(-1)
        n = self.num_classes if rows is None else int(rows.numel())
        out = torch.empty(n, self.num_classes, device=dev, dtype=torch.float32)
        if n == 0:
            return out
        a = L.TaxonomyRowsArgs()
        a.C, a.depth, a.anc, a.val, a.rows, a.n = self.num_classes, self.depth, _ptr(anc), _ptr(val), _ptr(rows), n
        a.out, a.ldo, a.what = _ptr(out), out.stride(0), what
        with torch.cuda.device(dev):
            L.check(L.lib().lnx_taxonomy_rows(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "lnx_taxonomy_rows")
        return out

    def dense(self, rows=None, device=None) -> torch.Tensor:
        """rows (all of them with rows=None) of the [C, C] soft-label matrix: build_taxonomy_smoothing_matrix on the device"""
        return self._rows(rows, device, 0)

    def distances(self, rows=None, device=None) -> torch.Tensor:
        """rows of the [C, C] distance matrix (2k, inf where disconnected, 0 on the diagonal): build_distance_matrix on the device"""
        return self._rows(rows, device, 1)


def _check_alpha_beta(alpha: float, beta: float) -> None:
    if not (0.0 <= alpha <= 1.0):
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    if beta < 0:
        raise ValueError(f"beta must be non-negative, got {beta}")


def build_taxonomy_smoothing_tables(parents, num_classes, level: int, alpha: float = 0.1, beta: float = 1.0, uniform_roots: bool = True,
                                    keep_fp64: bool = False) -> TaxonomySmoothingTables:
    """Tables of task level `level` (an index into `num_classes`, the class counts per level from the finest up).  `parents[l]` is an
    int array [num_classes[l]]: the index at level l + 1 of each class's parent, -1 for none -- the tree's hierarchy map; entries
    below `level` are not read, and a missing or empty top entry means no parents.  keep_fp64 also keeps `val64` (the unrounded
    values) and `counts` (int64 [C, D + 2]: how many classes of row i take each value) on the result."""
    import numpy as np

    _check_alpha_beta(alpha, beta)
    ncls = [int(c) for c in num_classes]
    if not 0 <= level < len(ncls):
        raise ValueError(f"level={level} outside the {len(ncls)} levels")
    Cn, D = ncls[level], len(ncls) - 1 - level
    if Cn <= 1:
        raise ValueError(f"taxonomy smoothing needs at least 2 classes, level {level} has {Cn} (the reference skips such tasks)")
    if D > TAX_MAX_DEPTH:
        raise L.LnxError(f"taxonomy tables hold at most {TAX_MAX_DEPTH} levels above the task's own (LNX_TAX_MAX_DEPTH), level {level} has {D}")
    anc = np.full((D, Cn), -1, np.int64)
    n = np.ones((D + 1, Cn), np.int64)
    prev = np.arange(Cn, dtype=np.int64)
    for k in range(1, D + 1):
        lv = level + k - 1
        p = parents[lv] if lv < len(parents) and parents[lv] is not None else None
        p = np.full(ncls[lv], -1, np.int64) if p is None or len(p) == 0 else np.asarray(p).astype(np.int64).reshape(-1)
        if p.shape[0] != ncls[lv]:
            raise ValueError(f"parents[{lv}] has {p.shape[0]} entries, level {lv} has {ncls[lv]} classes")
        if p.min() < -1 or p.max() >= ncls[lv + 1]:
            raise ValueError(f"parents[{lv}] holds a parent index outside [-1, {ncls[lv + 1] - 1}]")
        cur = np.where(prev >= 0, p[np.clip(prev, 0, None)], -1)
        cnt = np.bincount(cur[cur >= 0], minlength=ncls[lv + 1])
        n[k] = np.where(cur >= 0, cnt[np.clip(cur, 0, None)], n[k - 1])
        anc[k - 1] = prev = cur
    m = (n[1:] - n[:-1]).astype(np.float64)                        # [D, C] classes at distance 2k
    w = np.exp(-2.0 * float(beta) * np.arange(1, D + 1, dtype=np.float64))
    Z = (m * w[:, None]).sum(0) if D else np.zeros(Cn)
    root = anc[0] < 0 if D else np.ones(Cn, bool)
    uniform = (Z <= 1e-9) | (root & bool(uniform_roots))
    val = np.empty((Cn, D + 2), np.float64)
    val[:, 0] = 1.0 - alpha
    flat = alpha / (Cn - 1)
    safe = np.where(uniform, 1.0, Z)
    for k in range(1, D + 1):
        val[:, k] = np.where(uniform, flat, alpha * w[k - 1] / safe)
    val[:, D + 1] = np.where(uniform, flat, 0.0)
    counts = None
    if keep_fp64:
        counts = np.empty((Cn, D + 2), np.int64)
        counts[:, 0] = 1
        counts[:, 1:D + 1] = (n[1:] - n[:-1]).T
        counts[:, D + 1] = Cn - n[D]
    return TaxonomySmoothingTables(torch.from_numpy(anc.astype(np.int32)), torch.from_numpy(val.astype(np.float32)), alpha, beta,
                                   val64=val if keep_fp64 else None, counts=counts)


def _tree_parents(tree, first: int):
    """per-level parent arrays (None below `first`) of a duck-typed TaxonomyTree: task_keys, num_classes, get_nodes_at_level, get_parent"""
    import numpy as np

    keys = list(tree.task_keys)
    parents = [None] * len(keys)
    for lv in range(first, len(keys) - 1):
        nodes = tree.get_nodes_at_level(keys[lv])
        p = np.full(int(tree.num_classes[keys[lv]]), -1, np.int64)
        for i, node in enumerate(nodes):
            up = tree.get_parent(node)
            if up is not None and up[0] == keys[lv + 1]:
                p[i] = int(up[1])
        parents[lv] = p
    return parents


def taxonomy_smoothing_tables_from_tree(tree, task_key: str, alpha: float = 0.1, beta: float = 1.0, uniform_roots: bool = True,
                                        keep_fp64: bool = False) -> TaxonomySmoothingTables:
    """Tables of `task_key` from a TaxonomyTree-like object, read through `task_keys`, `num_classes`, `get_nodes_at_level` and
    `get_parent` only (the reference's class is never imported)."""
    keys = list(tree.task_keys)
    if task_key not in keys or task_key not in tree.num_classes:
        raise KeyError(f"Task key '{task_key}' not found in the taxonomy tree.")
    level = keys.index(task_key)
    return build_taxonomy_smoothing_tables(_tree_parents(tree, level), [int(tree.num_classes[k]) for k in keys], level, alpha, beta, uniform_roots,
                                           keep_fp64)


def generate_taxonomy_tables(config, taxonomy_tree, num_classes: Dict[str, int]) -> Dict[str, TaxonomySmoothingTables]:
    """{task: tables} with the per-task decisions of generate_taxonomy_matrices (utils/taxonomy/taxonomy_utils.py:24-254): only tasks
    whose LOSS.TAXONOMY_SMOOTHING.ENABLED flag is set; a task with unknown or <= 1 classes is skipped; a level none of whose classes
    has a parent is all-uniform (depth-0 tables) under FALLBACK_TO_UNIFORM and skipped without it; a level with parent links gets
    the distance-based tables (UNIFORM_ROOTS makes the parentless rows uniform); a task whose tables cannot be built (alpha or beta
    out of range, a class count that differs from the tree's) is skipped, as the reference skips a task whose matrix raises."""
    ts = config.LOSS.TAXONOMY_SMOOTHING
    task_keys, flags = list(config.DATA.TASK_KEYS_H5), list(ts.ENABLED)
    alpha, beta, uniform_roots, fallback = ts.ALPHA, ts.BETA, bool(ts.UNIFORM_ROOTS), bool(ts.FALLBACK_TO_UNIFORM)
    out = {}
    for i, task in enumerate(task_keys):
        if i >= len(flags) or not flags[i]:
            continue
        n = num_classes.get(task)
        if n is None or n <= 1:
            continue
        nodes = taxonomy_tree.get_nodes_at_level(task)
        has_parents = any(taxonomy_tree.get_parent(node) is not None for node in nodes)
        if not has_parents and not fallback:
            continue
        try:
            if not has_parents:  # (with parent links some class has a parent, so "all global roots" cannot hold: one uniform case)
                out[task] = build_taxonomy_smoothing_tables([], [int(n)], 0, alpha, beta, uniform_roots)
            elif int(taxonomy_tree.num_classes.get(task, -1)) != int(n):
                continue  # (the reference's distance matrix would not have the shape num_classes asks for: it skips the task)
            else:
                out[task] = taxonomy_smoothing_tables_from_tree(taxonomy_tree, task, alpha, beta, uniform_roots)
        except (ValueError, KeyError):
            continue
    return out


def _is_null(target: torch.Tensor) -> torch.Tensor:
    return target == 0 if target.dim() == 1 else target[:, 0] > 0.5


def _sorted_tasks(d):
    return sorted(d.keys(), key=lambda k: int(k.split("_L")[-1]))


def compute_core_loss(outputs, targets, criteria, config=None):
    """{task: per-sample loss [B]} in rank order; each criterion returns a [B] vector."""
    return {t: criteria[t](outputs[t], targets[t]) for t in _sorted_tasks(outputs)}


def _class_weight_vector(cw_dict, num_classes: int, device) -> torch.Tensor:
    v = torch.ones(num_classes, dtype=torch.float32)
    for i, w in cw_dict.items():
        if 0 <= int(i) < num_classes:
            v[int(i)] = float(w)
    return v.to(device)


def _sample_weights(cw_dict, target: torch.Tensor, cache: Optional[dict] = None, key=None) -> torch.Tensor:
    """per-sample class weight: cw[label] for hard labels, <soft target, cw> for [B, C] targets; missing classes weigh 1"""
    if target.dim() == 1:
        n = max(int(max(cw_dict.keys(), default=0)) + 1, 1)
        ck = (key, n, str(target.device))
        vec = cache.get(ck) if cache is not None else None
        if vec is None:
            vec = _class_weight_vector(cw_dict, n, target.device)
            if cache is not None:
                cache[ck] = vec
        idx = target.clamp(0, n - 1)
        return torch.where(target < n, vec[idx], torch.ones((), device=target.device))
    vec = _class_weight_vector(cw_dict, target.size(1), target.device)
    return (target.float() * vec.unsqueeze(0)).sum(1)


def apply_class_weighting(per_task_losses, targets, class_weights=None, _cache=None):
    if class_weights is None:
        return per_task_losses
    out = {}
    for t, vec in per_task_losses.items():
        out[t] = vec * _sample_weights(class_weights[t], targets[t], _cache, t).to(vec.dtype) if t in class_weights else vec
    return out


def apply_null_masking(per_task_losses, targets, null_mask_prob: float, logger=None, config=None, _coin=None):
    """Zero the loss of null-labelled samples (label 0) except for a random `null_mask_prob` fraction of them.
    Statistics are device scalars (the reference calls .item() on each).  `_coin`: {task: [B] uniform draws} for tests."""
    masked, stats = {}, {"null_mask_prob": null_mask_prob}
    tot = inc = None
    for t, vec in per_task_losses.items():
        null = _is_null(targets[t])
        if null_mask_prob < 1.0:
            u = _coin[t].to(vec.device) if _coin is not None else torch.rand(vec.shape[0], device=vec.device)
            keep = (~null) | (u < null_mask_prob)
        else:
            keep = torch.ones_like(null)
        masked[t] = torch.where(keep, vec, torch.zeros((), dtype=vec.dtype, device=vec.device))
        n, k = null.sum(), (null & keep).sum()
        tot, inc = (n, k) if tot is None else (tot + n, inc + k)
    stats["null_samples_total"], stats["null_samples_included"] = tot, inc
    stats["inclusion_percentage"] = inc.float() * 100.0 / tot.float().clamp_min(1.0) if tot is not None else 0.0
    return masked, stats


def apply_loss_masking(per_task_losses, targets, ops_schedule, current_step, class_weights=None, is_validation=False, logger=None, config=None,
                       _coin=None, _cache=None):
    if is_validation:
        prob = 1.0
    elif config is not None and getattr(config.TRAIN, "PHASE1_MASK_NULL_LOSS", False):
        prob = 0.0
    else:
        prob = float(ops_schedule.get_null_mask_prob(current_step))
    masked, stats = apply_null_masking(per_task_losses, targets, prob, logger, config, _coin)
    stats["num_valid_samples_per_task"] = {t: (v != 0).sum() for t, v in masked.items()}  # device scalars
    if class_weights is not None:
        return apply_class_weighting(masked, targets, class_weights, _cache), stats
    return masked, stats


def _cfg_get(node, path, default):
    for k in path.split("."):
        if node is None:
            return default
        node = node.get(k, None) if isinstance(node, dict) else getattr(node, k, None)
    return default if node is None else node


DEFAULT_EXCLUDE_CONFIG = {"TYPE": "or", "FILTERS": [{"TYPE": "name", "PATTERNS": ["head"]}, {"TYPE": "name", "PATTERNS": ["meta_"]}]}


def param_filter(spec) -> Callable[[str, torch.Tensor], bool]:
    """matches(name, param) of the reference's parameter filter config (utils/param_filters.py create_filter_from_config, as
    UnifiedParamFilter applies it: a leading 'module.' is stripped).  Types: name (contains / startswith / endswith / regex),
    dimension, and / or / not / all_except."""
    kind = str(_cfg_get(spec, "TYPE", "")).lower()
    if kind == "name":
        pats, how = list(_cfg_get(spec, "PATTERNS", [])), str(_cfg_get(spec, "MATCH_TYPE", "contains"))
        if how == "regex":
            rx = [re.compile(q) for q in pats]
            f = lambda n, p: any(r.search(n) for r in rx)  # noqa: E731
        elif how in ("contains", "startswith", "endswith"):
            f = {"contains": lambda n, p: any(q in n for q in pats), "startswith": lambda n, p: any(n.startswith(q) for q in pats),
                 "endswith": lambda n, p: any(n.endswith(q) for q in pats)}[how]
        else:
            raise ValueError(f"Unknown match_type: {how}")
    elif kind == "dimension":
        dims = list(_cfg_get(spec, "DIMENSIONS", []))
        f = lambda n, p: p.dim() in dims  # noqa: E731
    elif kind in ("and", "or"):
        subs = [param_filter(x) for x in _cfg_get(spec, "FILTERS", [])]
        f = (lambda n, p: all(g(n, p) for g in subs)) if kind == "and" else (lambda n, p: any(g(n, p) for g in subs))
    elif kind in ("not", "all_except"):
        sub = param_filter(_cfg_get(spec, "FILTER" if kind == "not" else "EXCEPT", {}))
        f = lambda n, p: not sub(n, p)  # noqa: E731
    else:
        raise ValueError(f"Unsupported filter type for the GradNorm backbone: {kind!r}")
    return lambda n, p: f(n[7:] if n.startswith("module.") else n, p)


class GradNormModule(nn.Module):
    """State of GradNorm (loss/gradnorm.py:31-140): buffers `task_weights` and `initial_losses` (same names as the reference, so
    state dicts load both ways), indexed by SORTED task key as measure_and_update does.  The update itself is lnx_gradnorm_update."""

    def __init__(self, task_keys, alpha: float = 1.5, init_weights: Optional[torch.Tensor] = None, label_densities=None, num_classes=None,
                 init_strategy: str = "inverse_density", config: Any = None):
        super().__init__()
        self.num_tasks = len(task_keys)
        self.task_keys = list(task_keys)
        self.alpha = float(alpha)
        self.config = config
        if init_weights is None:
            init_weights = self._compute_init_weights(self.task_keys, label_densities, num_classes, init_strategy)
        self.register_buffer("task_weights", torch.as_tensor(init_weights, dtype=torch.float32).clone())
        self.register_buffer("initial_losses", torch.zeros(self.num_tasks))
        self.register_buffer("_initted", torch.zeros(1, dtype=torch.int32), persistent=False)  # device twin of has_initted
        self.has_initted = False

    def _compute_init_weights(self, task_keys, label_densities=None, num_classes=None, strategy: str = "inverse_density") -> torch.Tensor:
        if not label_densities:
            return torch.ones(len(task_keys), dtype=torch.float32)
        dens = [label_densities.get(k, 1.0) for k in task_keys]
        if strategy == "inverse_density" or (strategy == "class_complexity" and num_classes is None):
            w = [1.0 / max(d, 0.001) for d in dens]
        elif strategy == "class_complexity":
            counts = [num_classes.get(k, 1) for k in task_keys]
            mx = max(counts)
            w = [1.0 / max(d, 0.001) * (math.log(c) / math.log(mx)) for d, c in zip(dens, counts)]
        else:
            w = [1.0] * len(task_keys)
        tot = sum(w)
        return torch.tensor([x * len(task_keys) / tot for x in w], dtype=torch.float32)

    def forward(self, losses):
        return (torch.stack([losses[k] for k in sorted(losses.keys())]) * self.task_weights).sum()

    def get_task_weights(self) -> Dict[str, float]:
        return {t: float(w) for t, w in zip(sorted(self.task_keys), self.task_weights.tolist())}


def backbone_slices(layout, backbone) -> list:
    """(offset, numel) in floats of every backbone parameter's slice of the gradient arena (`mFormerV1.grad_arena_layout()`), in
    arena order; `backbone` = the parameters (identity).  Parameters the plan does not differentiate are absent (zero gradient)."""
    ids = {id(p) for p in backbone}
    out = [(o, n) for o, n, p in zip(layout["offsets"], layout["numels"], layout["params"]) if id(p) in ids]
    return sorted(out)


def gradnorm_desc_table(slices, base_ptr: int):
    """lnx_adamw_desc table (only .g / .n / .block_start are read by lnx_gradnorm_sumsq) of arena slices at `base_ptr`, and its
    total workgroup count"""
    arr = (L.AdamWDesc * len(slices))()
    blk = 0
    for d, (off, n) in zip(arr, slices):
        d.g, d.n, d.group, d.block_start = base_ptr + 4 * off, n, 0, blk
        blk += (n + 4095) // 4096  # == lnx_adamw_blocks
    return arr, blk


class GradientWeighting(nn.Module):
    """Task weighting of the multi-task loss (loss/gradient_weighting.py:178-880): "static" (fixed weights) or "gradnorm".

    GradNorm: `set_model(model)` picks the shared backbone with LOSS.GRAD_WEIGHTING.TASK.EXCLUDE_CONFIG, and
    `update_gradnorm_weights_reforward` measures each task's backbone gradient norm and updates the weights.  Where the reference
    re-runs forward + autograd.grad per task, here ONE forward of the native plan feeds T backward passes into scratch gradient
    arenas (mFormerV1._task_backbone_grads); the norms (lnx_gradnorm_sumsq) and the update (lnx_gradnorm_update) stay on the
    device.  Reproduced from the reference: backbone .grad are set to None (opt out: keep_step_grads=True), weights indexed by
    sorted task key in the update but read in task_keys order by forward, initial weights from init_weights or ones."""

    def __init__(self, task_keys, config=None, task_weighting_type: str = "static", init_weights=None, class_weights=None,
                 use_subset_weights: bool = False, alpha: float = 1.5, label_densities=None, num_classes=None, init_strategy: str = "inverse_density",
                 update_interval: int = 100, exclude_patterns=None, zero_aux_info: bool = True, keep_step_grads: bool = False, **kwargs):
        super().__init__()
        if task_weighting_type not in ("static", "gradnorm"):
            raise NotImplementedError(f"task weighting type {task_weighting_type!r}: 'static' or 'gradnorm'")
        self.task_keys = list(task_keys)
        self.config = config
        self.task_weighting_type = task_weighting_type
        if isinstance(init_weights, dict):
            init_weights = [init_weights.get(k, 1.0) for k in self.task_keys]
        init_weights = list(init_weights or [1.0] * len(self.task_keys))
        self.task_weights = torch.tensor(init_weights, dtype=torch.float32)
        self.gradnorm = None
        self.update_interval, self.exclude_patterns = 0, []
        self.backbone_params = None
        self.model = None
        if task_weighting_type == "gradnorm":
            # the reference always hands GradNormModule a tensor: INIT_STRATEGY / label_densities never take effect
            self.gradnorm = GradNormModule(self.task_keys, alpha=alpha, init_weights=torch.tensor(init_weights, dtype=torch.float32),
                                           label_densities=label_densities, num_classes=num_classes, init_strategy=init_strategy, config=config)
            self.update_interval = update_interval
            self.exclude_patterns = exclude_patterns or ["head", "meta_"]
            self.zero_aux_info = bool(_cfg_get(config, "LOSS.GRAD_WEIGHTING.TASK.ZERO_AUX_INFO", zero_aux_info))
            self.keep_step_grads = bool(keep_step_grads)
        self.class_weights = class_weights
        self.use_subset_weights = use_subset_weights
        self._cache: dict = {}
        self._gn: dict = {}

    def _normalize_weights(self, w):
        return w

    # ------------------------------------------------------------------ GradNorm
    def set_model(self, model: nn.Module) -> None:
        if self.task_weighting_type != "gradnorm":
            return
        self.model = model
        net = model
        while hasattr(net, "module") and isinstance(net.module, nn.Module):  # torch DDP, linnaeus_amd.ddp.DataParallel
            net = net.module
        self._net = net
        spec = _cfg_get(self.config, "LOSS.GRAD_WEIGHTING.TASK.EXCLUDE_CONFIG", None) or DEFAULT_EXCLUDE_CONFIG
        f = param_filter(spec)
        self.backbone_names = [n for n, p in net.named_parameters() if p.requires_grad and not f(n, p)]
        self.backbone_params = [net.get_parameter(n) for n in self.backbone_names]
        self._gn = {}

    def scratch_arenas(self) -> int:
        """scratch gradient arenas one update holds (mFormerV1.plan_footprint(gradnorm_arenas=...))"""
        if self.gradnorm is None:
            return 0
        return 1 if int(_cfg_get(self.config, "LOSS.GRAD_WEIGHTING.TASK.GRADNORM_ACCUM_STEPS", 1)) <= 1 else len(self.task_keys)

    def _descs(self, arenas: torch.Tensor):
        """device descriptor table of the backbone slices of arena row 0, built once per arena layout"""
        net = self._net
        key = (arenas.data_ptr(), tuple(arenas.shape), net._arena_layout)
        if self._gn.get("key") != key:
            layout = net.grad_arena_layout()
            if layout["total"] != arenas.shape[1]:
                raise L.LnxError(f"gradient arena layout mismatch: {layout['total']} floats, scratch rows hold {arenas.shape[1]}")
            slices = backbone_slices(layout, self.backbone_params)
            if not slices:
                raise L.LnxError("GradNorm: no backbone parameter is differentiated by the model's plan")
            arr, blk = gradnorm_desc_table(slices, arenas.data_ptr())
            table = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(arenas.device)
            self._gn = {"key": key, "table": table, "ndesc": len(slices), "blocks": blk,
                        "ws": torch.empty(len(self.task_keys) * blk, device=arenas.device, dtype=torch.float32)}
        return self._gn

    def _sumsq(self, arenas, first: int, ntasks: int, norm: torch.Tensor, stream) -> None:
        g = self._descs(arenas)
        L.check(L.lib().lnx_gradnorm_sumsq(C.c_void_p(g["table"].data_ptr()), g["ndesc"], g["blocks"], ntasks, arenas.stride(0), None,
                                           C.c_void_p(norm.data_ptr() + 4 * first), C.c_void_p(g["ws"].data_ptr()), stream), "lnx_gradnorm_sumsq")

    def update_gradnorm_weights_reforward(self, data_batch, criteria, amp_enabled: bool = True, ops_schedule=None, current_step=None, *,
                                          sync: bool = True, keep_step_grads: Optional[bool] = None) -> Dict[str, Any]:
        """One GradNorm update (gradient_weighting.py:367-880) on `data_batch` = (images, {task: targets}, aux_info, ...).  The step's
        own gradients are not touched except that backbone .grad are set to None as in the reference (keep_step_grads=True: left
        alone).  Returns the reference's metrics: floats, or with sync=False device scalars (no host sync in the whole update)."""
        if self.task_weighting_type != "gradnorm" or self.gradnorm is None:
            return {}
        if self.model is None or not self.backbone_params:
            raise RuntimeError("GradientWeighting.set_model(model) must be called before a GradNorm update")
        net = self._net
        keep = self.keep_step_grads if keep_step_grads is None else bool(keep_step_grads)
        images, targets, aux = data_batch[0], data_batch[1], data_batch[2]
        dev = images.device
        aux_g = torch.zeros_like(aux) if (self.zero_aux_info and aux is not None) else aux
        S = max(1, int(_cfg_get(self.config, "LOSS.GRAD_WEIGHTING.TASK.GRADNORM_ACCUM_STEPS", 1)))
        ckpt = bool(_cfg_get(self.config, "TRAIN.GRADIENT_CHECKPOINTING.ENABLED_GRADNORM_STEPS", False))
        T = len(self.task_keys)
        plan_tasks = net._task_list()
        order = sorted(self.task_keys)  # measure_and_update's indexing
        if sorted(plan_tasks) != order:
            raise ValueError(f"GradNorm tasks {self.task_keys} differ from the model's heads {plan_tasks}")
        gn = self.gradnorm.to(dev)
        stats = torch.zeros(2, T, device=dev, dtype=torch.float32)  # loss_sum, valid count per plan task
        norm_plan = torch.zeros(T, device=dev, dtype=torch.float32)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        was_training = net.training
        net.train()
        try:
            B = images.shape[0]
            for s in range(S):
                lo = s * (B // S)
                hi = B if s == S - 1 else (s + 1) * (B // S)
                sb_t = {k: v[lo:hi].to(dev) for k, v in targets.items()}

                def seed(t, logits_t, dl_t, sb_t=sb_t):
                    name = plan_tasks[t]
                    y = sb_t[name]
                    valid = (y != 0) if y.dim() == 1 else (y[:, 0] <= 0.5)
                    cnt = valid.sum().float()
                    crit = criteria[name]
                    if isinstance(crit, TaxonomyAwareLabelSmoothingCE):
                        tgt = (y.argmax(dim=1) if y.dim() == 2 else y).to(torch.long).contiguous()
                        cw = crit.weight.to(dev) if (crit.apply_class_weights and crit.weight is not None) else None
                        rs = valid.float() / cnt.clamp_min(1.0)
                        per = torch.empty(y.shape[0], device=dev, dtype=torch.float32)
                        soft, form, tax = crit._row_source(dev)
                        _launch(_as_rows(logits_t), tgt, soft, 0.0, cw, crit.ignore_index, rs, 1.0, per, None, dl_t, form, None, None, tax)
                        lsum = torch.where(valid, per, torch.zeros((), device=dev)).sum()
                    else:  # any other criterion: autograd on a detached [B, C] leaf, never on the model
                        leaf = logits_t.detach().clone().requires_grad_(True)
                        with torch.enable_grad():
                            vec = crit(leaf, y)
                            lsum = vec[valid].sum()
                            g, = torch.autograd.grad(lsum / cnt.clamp_min(1.0), leaf, allow_unused=True)
                        if g is not None:
                            dl_t.copy_(g)
                        lsum = lsum.detach().float()
                    stats[0, t] += lsum
                    stats[1, t] += cnt

                after = None
                if S == 1:
                    after = lambda t: self._sumsq(net._gn_scratch, t, 1, norm_plan, stream)  # noqa: E731  (the one arena is reused)
                with torch.no_grad():
                    net._task_backbone_grads(images[lo:hi], aux_g[lo:hi] if aux_g is not None else None, seed, 1 if S == 1 else T, ckpt,
                                             accumulate=s > 0, after_task=after)
            if S > 1:
                self._sumsq(net._gn_scratch, 0, T, norm_plan, stream)
        finally:
            net.train(was_training)
        if self._gn.get("perm") is None or self._gn["perm"].device != dev:
            self._gn["perm"] = torch.tensor([plan_tasks.index(k) for k in order], device=dev)
        perm = self._gn["perm"]
        norm = norm_plan[perm]
        loss_sum, count = stats[0][perm].contiguous(), stats[1][perm].contiguous()
        init_loss = None
        distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
        if distributed:  # the reference all-reduces each norm (and, once, each loss) and divides by the world size
            ws = dist.get_world_size()
            dist.all_reduce(norm)
            norm = norm / ws
            if gn.alpha > 0 and not gn.has_initted:
                init_loss = loss_sum / count.clamp_min(1.0)
                dist.all_reduce(init_loss)
                init_loss = init_loss / ws
        metrics = torch.empty(1 + 5 * T, device=dev, dtype=torch.float32)
        a = L.GradNormArgs()
        a.T, a.alpha = T, gn.alpha
        a.norm, a.loss_sum, a.count = norm.data_ptr(), loss_sum.data_ptr(), count.data_ptr()
        a.init_loss = init_loss.data_ptr() if init_loss is not None else None
        a.weights, a.initial_losses, a.initted, a.metrics = gn.task_weights.data_ptr(), gn.initial_losses.data_ptr(), gn._initted.data_ptr(), metrics.data_ptr()
        L.check(L.lib().lnx_gradnorm_update(C.byref(a), stream), "lnx_gradnorm_update")
        if gn.alpha > 0:
            gn.has_initted = True
        self._gn_keepalive = (norm, loss_sum, count, init_loss, stats, norm_plan)  # (the launches above read them)
        if not keep:
            for p_ in self.backbone_params:
                p_.grad = None
        vals = metrics.tolist() if sync else metrics
        out = {"gradnorm/avg_norm": vals[0]}
        kinds = ("loss", "norm", "target", "weight") + (("ratio",) if gn.alpha > 0 else ())
        for j, kind in enumerate(kinds):
            for i, k in enumerate(order):
                out[f"gradnorm/{kind}/{k}"] = vals[1 + j * T + i]
        return out

    def forward(self, per_task_losses, targets, subset_ids=None, mixed_subset_ids=None, num_valid_samples_per_task=None):
        first = next(iter(per_task_losses.values()))
        if self.gradnorm is not None:
            norm_w = self.gradnorm.task_weights.to(device=first.device, dtype=first.dtype)  # task_keys order, as the reference reads it
        else:
            norm_w = self._normalize_weights(self.task_weights)
        weighted = {}
        for i, t in enumerate(self.task_keys):
            vec = per_task_losses[t]
            nv = vec.shape[0]
            if num_valid_samples_per_task is not None:
                nv = num_valid_samples_per_task.get(t, vec.shape[0])
            if self.class_weights and t in self.class_weights:
                vec = vec * _sample_weights(self.class_weights[t], targets[t], self._cache, t).to(vec.dtype)
            denom = nv.to(vec.dtype).clamp_min(1e-6) if isinstance(nv, torch.Tensor) else max(float(nv), 1e-6)
            weighted[t] = vec.sum() / denom * (norm_w[i] if self.gradnorm is not None else float(norm_w[i]))
        if self.gradnorm is not None:  # device scalars: no host sync in the step
            return weighted, {t: norm_w[i] for i, t in enumerate(self.task_keys)}
        return weighted, dict(zip(self.task_keys, norm_w.tolist()))


def weighted_hierarchical_loss(outputs, targets, criteria, task_weighting, ops_schedule, current_step: int, subset_ids=None, mixed_subset_ids=None,
                               is_validation: bool = False, logger=None, config=None, *, sync_components: bool = True, _coin=None, fused: bool = False):
    """(total_loss, loss_components, task_weights) of the reference's train / validation step.  With
    `sync_components=False` the logging values stay device scalars (no host sync in the step).  `fused=True` runs the same
    function as FusedHierarchicalLoss (three launches whatever the number of tasks), built once and kept on `task_weighting`."""
    if fused:
        cached = getattr(task_weighting, "_fused_loss", None)
        if cached is None or cached[0] is not criteria or cached[1] is not config:
            cached = (criteria, config, FusedHierarchicalLoss(task_weighting.task_keys, criteria, task_weighting, config))
            task_weighting._fused_loss = cached  # rebuilt when another criteria dict or config object is passed
        return cached[2](outputs, targets, ops_schedule, current_step, is_validation=is_validation, sync_components=sync_components, _coin=_coin)
    keys = _sorted_tasks(outputs)
    if not isinstance(targets, dict):
        targets = dict(zip(keys, targets))
    per = compute_core_loss(outputs, targets, criteria, config)
    raw = {k: v.detach().clone() for k, v in per.items()}
    phase1 = bool(config is not None and getattr(config.TRAIN, "PHASE1_MASK_NULL_LOSS", False))
    cache = getattr(task_weighting, "_cache", None)
    if phase1 and not is_validation:
        masked = {t: v * (~_is_null(targets[t])).to(v.dtype) for t, v in per.items()}
        zero = torch.zeros((), device=next(iter(per.values())).device)
        stats = {"null_samples_total": zero, "null_samples_included": zero, "inclusion_percentage": 0.0, "null_mask_prob": 0.0}
    else:
        masked, stats = apply_loss_masking(per, targets, ops_schedule, current_step, task_weighting.class_weights, is_validation, logger, config,
                                           _coin=_coin, _cache=cache)
    stats["phase1_active"] = phase1 and not is_validation
    after_cw = masked
    if task_weighting.class_weights:
        try:
            apply_cw = config.LOSS.GRAD_WEIGHTING.CLASS.TRAIN if not is_validation else config.LOSS.GRAD_WEIGHTING.CLASS.VAL
        except Exception:
            apply_cw = True
        if apply_cw:
            after_cw = apply_class_weighting(masked, targets, task_weighting.class_weights, cache)
    weighted, task_weights = task_weighting(after_cw, targets, num_valid_samples_per_task=stats.get("num_valid_samples_per_task", {}))
    total = sum(weighted.values())
    val = (lambda x: x.item()) if sync_components else (lambda x: x.detach())
    comps = {"total": val(total), "tasks": {t: val(per[t].mean()) for t in keys}, "masked_tasks": {t: val(after_cw[t].mean()) for t in keys},
             "weighted_tasks": {t: val(weighted[t]) for t in keys}, "raw_per_sample_losses": raw, "null_masking": stats}
    return total, comps, task_weights


# ----------------------------------------------------------------------------------------------------------------------
# The same function in a fixed number of launches (lnx_hier_loss_fwd / lnx_hier_loss_bwd, csrc/hier_loss.hip): two forward, one
# backward, whatever the number of tasks and the batch size, and no host synchronisation.  What the composed path above decides with
# Python conditions per step, class_weight_powers() decides once per call into two small integers per task.
# ----------------------------------------------------------------------------------------------------------------------
def class_weight_powers(task_weighting, config, is_validation: bool, task: str):
    """(p_cw, p_w): how often the composed path multiplies `task`'s per-sample class weight into the loss it logs as
    masked_tasks, and into the weighted loss (finding F13).  apply_loss_masking multiplies once unless the PHASE1 training branch
    skips it; weighted_hierarchical_loss once more under LOSS.GRAD_WEIGHTING.CLASS.TRAIN / .VAL (True when the config has no such
    node); GradientWeighting.forward once more in the weighted loss only."""
    cw = task_weighting.class_weights
    if not cw or task not in cw:
        return 0, 0
    phase1 = bool(config is not None and getattr(config.TRAIN, "PHASE1_MASK_NULL_LOSS", False)) and not is_validation
    try:
        apply_cw = config.LOSS.GRAD_WEIGHTING.CLASS.TRAIN if not is_validation else config.LOSS.GRAD_WEIGHTING.CLASS.VAL
    except Exception:
        apply_cw = True
    p_cw = (0 if phase1 else 1) + (1 if apply_cw else 0)
    return p_cw, p_cw + 1


class _HierLoss(torch.autograd.Function):
    """total loss of all tasks; the gradients of all tasks are views of one flat buffer that one launch fills"""

    @staticmethod
    def forward(ctx, owner, call, *logits):
        a, keep, out = call
        st = C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
        L.check(L.lib().lnx_hier_loss_fwd(C.byref(a), st), "lnx_hier_loss_fwd")
        ctx.call = call
        ctx.meta = [(lg.shape, lg.dtype, lg.requires_grad) for lg in logits]
        return out[L.HL_OUT_TOTAL]

    @staticmethod
    def backward(ctx, go):
        a, keep, out = ctx.call
        sizes = [shp[0] * shp[1] if need else 0 for shp, _, need in ctx.meta]
        if not any(sizes):
            return (None, None) + (None,) * len(sizes)
        flat = torch.empty(sum(sizes), device=out.device, dtype=torch.float32)
        grads, off = [], 0
        for i, ((shp, dt, need), n) in enumerate(zip(ctx.meta, sizes)):
            d = flat[off:off + n].view(shp) if n else None
            off += n
            a.task[i].dlogits, a.task[i].ldd = _ptr(d), (shp[1] if n else 0)
            grads.append(d)
        go = go.to(torch.float32).contiguous()
        st = C.c_void_p(torch.cuda.current_stream(out.device).cuda_stream)
        L.check(L.lib().lnx_hier_loss_bwd(C.byref(a), _ptr(go), st), "lnx_hier_loss_bwd")
        if any(dt != torch.float32 for _, dt, need in ctx.meta if need):  # bf16 logits: one cast of the flat buffer per storage type
            cast = {dt: flat.to(dt) for _, dt, need in ctx.meta if need and dt != torch.float32}
            off = 0
            for i, ((shp, dt, need), n) in enumerate(zip(ctx.meta, sizes)):
                if n and dt != torch.float32:
                    grads[i] = cast[dt][off:off + n].view(shp)
                off += n
        return (None, None) + tuple(grads)


class FusedHierarchicalLoss:
    """weighted_hierarchical_loss (above; loss/hierarchical_loss.py:24-406) as lnx_hier_loss_fwd / lnx_hier_loss_bwd: criterion, null
    masking, class weighting with finding F13's multiplicities, valid-sample denominators, static or GradNorm task weights, the total,
    every logged component and the null statistics in two launches, the gradients of every task's logits in one more.

    Supported criteria, in any mix over up to 8 tasks: TaxonomyAwareLabelSmoothingCE (over its matrix, or in table form), this module's CrossEntropyLoss,
    LabelSmoothingCrossEntropy and SoftTargetCrossEntropy (with their class weights, uploaded once, and [B] or [B, C] targets; [B, C] only
    for SoftTargetCrossEntropy), and torch.nn.CrossEntropyLoss(reduction="none", label_smoothing=eps) without a class weight of its own
    and with [B] targets.  Anything else, dict-valued head outputs and CPU tensors are refused by name (LnxError): there is no fall-back
    to the composed path."""

    def __init__(self, task_keys, criteria, task_weighting, config=None):
        self.task_keys = list(task_keys)
        if not 1 <= len(self.task_keys) <= SOFTCE_MAX_TASKS:
            raise L.LnxError(f"FusedHierarchicalLoss: {len(self.task_keys)} tasks (1..{SOFTCE_MAX_TASKS})")
        if list(task_weighting.task_keys) != self.task_keys:
            raise L.LnxError(f"FusedHierarchicalLoss: task_keys {self.task_keys} differ from the task weighting's {list(task_weighting.task_keys)}")
        self.criteria, self.task_weighting, self.config = criteria, task_weighting, config
        self._crit = {}
        for t in self.task_keys:
            if t not in criteria:
                raise L.LnxError(f"FusedHierarchicalLoss: no criterion for task {t!r}")
            crit = criteria[t]
            if isinstance(crit, TaxonomyAwareLabelSmoothingCE):
                self._crit[t] = "soft"
            elif type(crit) is nn.CrossEntropyLoss:
                if crit.reduction != "none":
                    raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: CrossEntropyLoss(reduction={crit.reduction!r}) is not supported (per-sample losses need reduction='none')")
                if crit.weight is not None:
                    raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: CrossEntropyLoss with a class weight is not supported")
                if not 0.0 <= float(crit.label_smoothing) < 1.0:
                    raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: label_smoothing={crit.label_smoothing} outside [0, 1)")
                self._crit[t] = "ce"
            elif isinstance(crit, _BasicCriterion):
                if isinstance(crit, LabelSmoothingCrossEntropy) and not 0.0 <= float(crit.smoothing) < 1.0:
                    raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: smoothing={crit.smoothing} outside [0, 1)")
                self._crit[t] = "basic"
            else:
                raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: criterion {type(crit).__name__} is not supported ({ACCEPTED_CRITERIA})")
        self._dev = None
        self._cw = {}      # task -> (device vector, length): uploaded once
        self._critw = {}   # task -> [C] class weight of a CrossEntropyLoss / LabelSmoothingCrossEntropy / SoftTargetCrossEntropy: uploaded once
        self._static_w = None
        self._draws = {}   # (n_tasks, B) -> [n_tasks, B] buffer of uniform draws
        for crit in criteria.values():  # upload at construction when the criteria already live on a GPU
            sl = getattr(crit, "soft_labels", None)
            if sl is None:
                sl = getattr(crit, "tax_val", None)  # (a TaxonomyAwareLabelSmoothingCE in table form)
            if isinstance(sl, torch.Tensor) and sl.is_cuda:
                self._prepare(sl.device)
                break

    def _prepare(self, dev):
        """what does not change from step to step: class-weight vectors, static task weights, the criteria's buffers on `dev`"""
        self._dev = dev
        tw = self.task_weighting
        self._cw = {}
        self._critw = {}
        for t in self.task_keys:
            crit = self.criteria[t]
            if self._crit[t] == "basic" and crit.weight is not None and crit.apply_class_weights:
                w = crit.weight if isinstance(crit.weight, torch.Tensor) else torch.tensor(crit.weight, dtype=torch.float32)
                self._critw[t] = w.detach().to(dev, torch.float32).contiguous()
            if self._crit[t] == "soft":
                crit._row_source(dev)
                if crit.apply_class_weights and crit.weight is not None and crit.weight.device != dev:
                    crit.weight = crit.class_weight = crit.weight.to(dev)
            if tw.class_weights and t in tw.class_weights:
                d = tw.class_weights[t]
                nc = crit.num_classes if self._crit[t] == "soft" else 0
                n = max(int(max(d.keys(), default=0)) + 1, 1, nc)  # (entries past _sample_weights' vector are its default, 1)
                self._cw[t] = (_class_weight_vector(d, n, dev), n)
        if tw.gradnorm is None:
            self._static_w = tw._normalize_weights(tw.task_weights).to(torch.float32).to(dev)
            self._static_w_host = dict(zip(self.task_keys, tw._normalize_weights(tw.task_weights).tolist()))
        elif tw.gradnorm.task_weights.device != dev:
            tw.gradnorm.to(dev)

    def __call__(self, outputs, targets, ops_schedule, current_step, is_validation: bool = False, sync_components: bool = False, _coin=None):
        keys = _sorted_tasks(outputs)
        if sorted(keys) != sorted(self.task_keys):
            raise L.LnxError(f"FusedHierarchicalLoss: outputs hold tasks {keys}, built for {self.task_keys}")
        if not isinstance(targets, dict):
            targets = dict(zip(keys, targets))
        for t in keys:
            if isinstance(outputs[t], dict):
                raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: dict-valued head outputs (ConditionalClassifierHead refinement) are not supported")
            if not isinstance(outputs[t], torch.Tensor) or outputs[t].dim() != 2:
                raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: logits must be a [B, C] tensor")
            if not outputs[t].is_cuda or not targets[t].is_cuda:
                raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: CPU tensors are not supported (logits and targets must be on the GPU)")
        first = outputs[self.task_keys[0]]
        dev, B, dtype = first.device, first.shape[0], first.dtype
        if dtype not in (torch.float32, torch.bfloat16):
            raise L.LnxError(f"FusedHierarchicalLoss: logits dtype {dtype} is not supported (float32 or bfloat16)")
        if self._dev != dev:
            self._prepare(dev)
        config, tw, T = self.config, self.task_weighting, len(self.task_keys)
        phase1 = bool(config is not None and getattr(config.TRAIN, "PHASE1_MASK_NULL_LOSS", False))
        p1_train = phase1 and not is_validation
        if is_validation:
            prob = 1.0
        elif phase1:
            prob = 0.0
        else:
            prob = float(ops_schedule.get_null_mask_prob(current_step))

        # one allocation per call for everything the launches write (the caching allocator: no launch, no synchronisation); the
        # per-sample losses handed back and the rows the backward reads live in it, so a later call never overwrites them
        buf = torch.empty(2 * L.HL_COUNTS + L.HL_OUT_FLOATS + L.HL_WS_ROWS * T * B, device=dev, dtype=torch.float32)
        counts = buf[:2 * L.HL_COUNTS].view(torch.int64)
        out = buf[2 * L.HL_COUNTS:2 * L.HL_COUNTS + L.HL_OUT_FLOATS]
        ws = buf[2 * L.HL_COUNTS + L.HL_OUT_FLOATS:].view(T, L.HL_WS_ROWS, B)
        draws = None
        if 0.0 < prob < 1.0:
            draws = self._draws.get((T, B))
            if draws is None or draws.device != dev:
                draws = self._draws[(T, B)] = torch.empty(T, B, device=dev, dtype=torch.float32)
            for t in keys:  # in the composed path's order, so that the same seed keeps the same rows
                row = draws[self.task_keys.index(t)]
                if _coin is not None:
                    row.copy_(_coin[t])
                else:
                    torch.rand(B, out=row)
        weights = tw.gradnorm.task_weights if tw.gradnorm is not None else self._static_w

        a = L.HierLossArgs()
        a.dtype, a.B, a.n_tasks = (L.BF16 if dtype == torch.bfloat16 else L.F32), B, T
        a.prob, a.mask_mul = prob, int(p1_train)
        a.draws, a.weights = _ptr(draws), _ptr(weights)
        a.ws, a.out, a.counts = _ptr(ws), _ptr(out), _ptr(counts)
        keep = [buf, draws, weights]  # what the launches read or write must outlive them
        logits = []
        for i, t in enumerate(self.task_keys):
            x, y, crit, k = outputs[t], targets[t], self.criteria[t], a.task[i]
            if x.shape[0] != B or x.dtype != dtype:
                raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: logits {tuple(x.shape)} {x.dtype}, the first task has batch {B} and {dtype}")
            if x.stride(1) != 1:
                x = x.contiguous()
            k.logits, k.ld, k.C = _ptr(x), x.stride(0), x.shape[1]
            if self._crit[t] == "soft":
                if x.shape[1] != crit.num_classes:
                    raise ValueError(f"Logits dimension mismatch. Expected {crit.num_classes} classes, got {x.shape[1]}.")
                soft, k.form, tax = crit._row_source(dev)
                k.soft, k.smoothing = _ptr(soft), 0.0
                if tax is not None:
                    k.tax_anc, k.tax_val, k.tax_depth = _ptr(tax[0]), _ptr(tax[1]), int(tax[2])
                k.crit_weight = _ptr(crit.weight) if (crit.apply_class_weights and crit.weight is not None) else None
                k.ignore_index = -1 if crit.ignore_index is None else int(crit.ignore_index)
            elif self._crit[t] == "basic":
                w = self._critw.get(t)
                if w is not None and (w.dim() != 1 or w.numel() != x.shape[1]):
                    raise ValueError(f"{type(crit).__name__}: weight has {tuple(w.shape)} entries, the logits have {x.shape[1]} classes")
                if crit._form == L.CE_FORM_SOFT_ROW and (y.dim() != 2 or y.shape[1] != x.shape[1]):
                    raise ValueError(f"SoftTargetCrossEntropy needs [B, C] targets of the logits' shape {tuple(x.shape)}, got {tuple(y.shape)}")
                k.form, k.soft, k.crit_weight = crit._form, None, _ptr(w)
                k.smoothing = float(crit.smoothing) if crit._form == L.CE_FORM_OFF_TARGET else 0.0
                ign = getattr(crit, "ignore_index", None)
                k.ignore_index = int(ign) if (ign is not None and ign >= 0) else -1
            else:
                if y.dim() != 1:
                    raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: torch.nn.CrossEntropyLoss with [B, C] targets is not supported")
                k.soft, k.smoothing, k.crit_weight = None, float(crit.label_smoothing), None
                k.ignore_index = int(crit.ignore_index) if crit.ignore_index >= 0 else -1
            if y.dim() == 1:
                y = y.to(torch.long).contiguous()
                k.target, k.soft_target, k.ldt = _ptr(y), None, 0
            elif y.dim() == 2 and y.shape[1] == x.shape[1]:
                y = y.float()
                if y.stride(1) != 1:
                    y = y.contiguous()
                k.target, k.soft_target, k.ldt = None, _ptr(y), y.stride(0)
            else:
                raise ValueError(f"Target tensor has invalid shape {tuple(y.shape)}. Expected 1D indices or [B, C] one-hot/soft-representing-one-class.")
            if y.shape[0] != B:
                raise L.LnxError(f"FusedHierarchicalLoss: task {t!r}: {y.shape[0]} targets for a batch of {B}")
            k.p_cw, k.p_w = class_weight_powers(tw, config, is_validation, t)
            if t in self._cw and k.p_w:
                if y.dim() == 2 and self._cw[t][1] < x.shape[1]:  # [B, C] targets read every class: the missing ones weigh 1 (rebuilt once)
                    self._cw[t] = (_class_weight_vector(tw.class_weights[t], x.shape[1], dev), x.shape[1])
                k.class_weight, k.n_cw = _ptr(self._cw[t][0]), self._cw[t][1]
            else:
                k.class_weight, k.n_cw = None, 0
            k.dlogits, k.ldd = None, 0
            keep += [x, y]
            logits.append(outputs[t])

        call = (a, keep, out)
        if torch.is_grad_enabled() and any(lg.requires_grad for lg in logits):
            total = _HierLoss.apply(self, call, *logits)
        else:
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            L.check(L.lib().lnx_hier_loss_fwd(C.byref(a), st), "lnx_hier_loss_fwd")
            total = out[L.HL_OUT_TOTAL]

        idx = {t: i for i, t in enumerate(self.task_keys)}
        M = SOFTCE_MAX_TASKS
        stats = {}
        if p1_train:
            zero = torch.zeros((), device=dev)
            stats.update(null_samples_total=zero, null_samples_included=zero, inclusion_percentage=0.0, null_mask_prob=0.0)
        else:
            stats.update(null_mask_prob=prob, null_samples_total=counts[L.HL_NULL_TOTAL], null_samples_included=counts[L.HL_NULL_INCLUDED],
                         inclusion_percentage=out[L.HL_OUT_INCLUSION], num_valid_samples_per_task={t: counts[idx[t]] for t in keys})
        stats["phase1_active"] = p1_train
        if sync_components:  # one read of the 40 floats
            host = out.tolist()
            val = lambda j: host[j]  # noqa: E731
        else:
            det = out.detach()
            val = lambda j: det[j]  # noqa: E731
        comps = {"total": val(L.HL_OUT_TOTAL), "tasks": {t: val(L.HL_OUT_RAW_MEAN * M + idx[t]) for t in keys},
                 "masked_tasks": {t: val(L.HL_OUT_MASKED_MEAN * M + idx[t]) for t in keys},
                 "weighted_tasks": {t: val(L.HL_OUT_WEIGHTED * M + idx[t]) for t in keys},
                 "raw_per_sample_losses": {t: ws[idx[t], L.HL_WS_RAW] for t in keys}, "null_masking": stats}
        if tw.gradnorm is not None:
            task_weights = {t: weights[i] for i, t in enumerate(self.task_keys)}
        else:
            task_weights = dict(self._static_w_host)
        return total, comps, task_weights
