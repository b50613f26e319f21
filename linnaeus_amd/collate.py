"""GPU-side batch mixing and metadata masking of the collate step: the reference's group-aware
selective Mixup and CutMix with the same call signature and results, and its scheduled full / partial metadata masking, as HIP
launches (csrc/collate.hip) instead of per-sample Python.

  GPUSelectiveMixup   <- linnaeus/aug/gpu/selective_mixup.py:14-604
  GPUSelectiveCutMix  <- linnaeus/aug/gpu/selective_cutmix.py:22-543
  GPUMetaMasking      <- linnaeus/h5data/h5dataloader.py:709-940, ops_schedule/ops_schedule.py:450-650
  mask_meta_components <- linnaeus/validation.py:174-175, 428-489
  GPUTrainCollate     <- linnaeus/h5data/h5dataloader.py:642-1801 (the training half of collate_fn)
  exclude_null_samples_from_mixup <- linnaeus/aug/utils.py:46-180
  rand_bbox           <- linnaeus/aug/utils.py:16-43

`batch = (images [B,C,H,W] fp32, targets {task: [B,Cn] soft labels or [B] indices}, aux_info [B,D], meta_validity_masks
[B,D] bool, group_ids [B])`; returns `(mixed_images, mixed_targets, mixed_aux_info, mixed_meta_valids)`.
What differs from the reference is only the mechanics: the in-group permutation is two segmented shuffles on the device
(no per-group Python loop), the metadata "hard pick" is one kernel (the reference loops over samples and chunks with a
host sync each), the probability / lambda / box draws come from the host generator (no `.item()` on a device tensor),
and the caller's aux_info is not modified in place.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math
import random
from typing import Any, Dict, List, Optional, Tuple

import torch

from . import _lib as L


def rand_bbox(size, lam: float) -> Tuple[int, int, int, int]:
    """(bbx1, bby1, bbx2, bby2): the reference names size[2] "W" and cuts [.., bbx1:bbx2, bby1:bby2]"""
    Wd, Hd = size[2], size[3]
    cut = math.sqrt(1.0 - lam)
    cw, ch = int(Wd * cut), int(Hd * cut)
    cx, cy = random.randint(0, Wd), random.randint(0, Hd)
    return max(0, cx - cw // 2), max(0, cy - ch // 2), min(Wd, cx + cw // 2), min(Hd, cy + ch // 2)


def exclude_null_samples_from_mixup(batch, null_task_keys=None, config=None):
    """group_id -> -1 for samples whose label is null (index 0 / one-hot column 0 > 0.5) in any of the checked tasks"""
    images, targets, aux, masks, gids = batch
    keys = list(targets.keys()) if null_task_keys is None else ([null_task_keys] if isinstance(null_task_keys, str) else list(null_task_keys))
    null = torch.zeros_like(gids, dtype=torch.bool)
    for k in keys:
        if k in targets:
            t = targets[k].to(gids.device)
            null |= (t == 0) if t.dim() == 1 else (t[:, 0] > 0.5)
    return images, targets, aux, masks, torch.where(null, torch.full_like(gids, -1), gids)


def ingroup_permutation(group_ids: torch.Tensor) -> torch.Tensor:
    """Uniform random permutation inside every group of size > 1 (group -1: identity), without host round trips: two
    independent random orders of each group's members are aligned position by position."""
    B = group_ids.numel()
    g = group_ids.to(torch.int64)
    key = g * 2 * B  # group-major; the random tie-break stays inside the group
    o1 = torch.argsort(key + torch.argsort(torch.rand(B, device=g.device)), stable=True)
    o2 = torch.argsort(key + torch.argsort(torch.rand(B, device=g.device)), stable=True)
    perm = torch.empty(B, dtype=torch.int64, device=g.device)
    perm[o1] = o2
    ar = torch.arange(B, device=g.device)
    return torch.where(g == -1, ar, perm)


def _mix_rows(x: torch.Tensor, perm: torch.Tensor, lam: float, mode: int, valid: Optional[torch.Tensor] = None, box=None, hw=None) -> torch.Tensor:
    if not x.is_cuda:
        raise L.LnxError("linnaeus_amd.collate runs on the HIP kernels only: move the batch to the GPU first")
    xf = x.float().contiguous()
    B = xf.shape[0]
    row = xf[0].numel()
    pad = (-row) % 4
    if pad:  # ragged class counts: pad the row (mode 1 never needs it: W % 4 == 0 is required there)
        xf = torch.nn.functional.pad(xf.reshape(B, row), (0, pad))
    out = torch.empty_like(xf)
    a = L.MixArgs()
    a.x, a.perm, a.out = xf.data_ptr(), perm.data_ptr(), out.data_ptr()
    vb = valid.to(torch.uint8).contiguous() if valid is not None else None
    a.valid = vb.data_ptr() if vb is not None else None
    a.B, a.row, a.lam, a.mode = B, row + pad, float(lam), mode
    if mode == 1:
        a.H, a.W = hw
        a.h0, a.h1, a.w0, a.w1 = box
    L.check(L.lib().lnx_mix_rows(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_mix_rows")
    if pad:
        out = out[:, :row]
    return out.reshape(x.shape).to(x.dtype if x.is_floating_point() else torch.float32)


class _SelectiveMixBase:
    def __init__(self, mix_config: Dict[str, Any], config=None):
        self.mix_config = mix_config
        self.config = config
        b = mix_config.get("meta_chunk_bounds_list")
        self.chunk_bounds: Optional[List[Tuple[int, int]]] = [tuple(x) for x in b] if isinstance(b, list) else None
        self.last_permutation = None
        self._bounds_dev = {}
        self._inject = None  # tests: dict(perm=, lam=, pick=, box=) recorded from the reference run

    def _mix_meta(self, aux: torch.Tensor, masks: torch.Tensor, perm: torch.Tensor, pick: Optional[torch.Tensor]):
        B, D = aux.shape
        if D == 0:
            return aux.clone(), masks.clone()
        bounds = self.chunk_bounds if self.chunk_bounds is not None else [(0, D)]
        key = (tuple(bounds), str(aux.device))
        bd = self._bounds_dev.get(key)
        if bd is None:
            bd = self._bounds_dev[key] = torch.tensor([v for se in bounds for v in se], dtype=torch.int32, device=aux.device)
        if pick is None:
            pick = torch.rand(B, device=aux.device)
        af = aux.float().contiguous()
        mk = masks.to(torch.uint8).contiguous()
        oa, om = torch.empty_like(af), torch.empty_like(mk)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L.check(L.lib().lnx_mix_meta(C.c_void_p(af.data_ptr()), C.c_void_p(mk.data_ptr()), C.c_void_p(perm.data_ptr()), C.c_void_p(pick.float().contiguous().data_ptr()),
                                     C.c_void_p(bd.data_ptr()), len(bounds), B, D, C.c_void_p(oa.data_ptr()), C.c_void_p(om.data_ptr()), st), "lnx_mix_meta")
        # columns outside every chunk keep the sample's own values (the reference leaves them uninitialised)
        covered = torch.zeros(D, dtype=torch.bool, device=aux.device)
        for s, e in bounds:
            covered[s:e] = True
        if not bool(covered.all()):
            oa = torch.where(covered, oa, af)
            om = torch.where(covered, om, mk)
        return oa.to(aux.dtype), om.to(masks.dtype)

    def _prologue(self, batch, exclude_null_samples, null_task_keys):
        if exclude_null_samples:
            batch = exclude_null_samples_from_mixup(batch, null_task_keys, config=self.config)
        return batch

    def _perm(self, gids):
        perm = self._inject["perm"].to(gids.device) if self._inject else ingroup_permutation(gids)
        self.last_permutation = perm
        return perm.contiguous()


class GPUSelectiveMixup(_SelectiveMixBase):
    """mix_config: {"PROB", "ALPHA", "meta_chunk_bounds_list"} (linnaeus/aug/gpu/selective_mixup.py:29-45)"""

    def __call__(self, batch, exclude_null_samples: bool = True, null_task_keys=None):
        images, targets, aux, masks, gids = self._prologue(batch, exclude_null_samples, null_task_keys)
        inj = self._inject
        if inj is None and random.random() > self.mix_config["PROB"]:
            return images, targets, aux, masks
        if bool((gids == -1).all()):
            return images, targets, aux, masks
        perm = self._perm(gids)
        alpha = self.mix_config["ALPHA"]
        lam = float(inj["lam"]) if inj else float(torch.distributions.beta.Beta(alpha, alpha).sample())
        mixed_images = _mix_rows(images, perm, lam, 0)
        mixed_targets = {k: _mix_rows(v, perm, lam, 0) for k, v in targets.items()}
        mixed_aux, mixed_masks = self._mix_meta(aux, masks, perm, inj["pick"].to(aux.device) if inj else None)
        return mixed_images, mixed_targets, mixed_aux, mixed_masks


class GPUSelectiveCutMix(_SelectiveMixBase):
    """mix_config: {"PROB", "ALPHA", "MINMAX", "meta_chunk_bounds_list"} (linnaeus/aug/gpu/selective_cutmix.py:40-90)"""

    def __init__(self, mix_config, config=None):
        super().__init__(mix_config, config)
        self.minmax = mix_config.get("MINMAX", None)

    def __call__(self, batch, exclude_null_samples: bool = True, null_task_keys=None):
        images, targets, aux, masks, gids = self._prologue(batch, exclude_null_samples, null_task_keys)
        inj = self._inject
        if inj is None and random.random() > self.mix_config.get("PROB", 1.0):
            return images, targets, aux, masks
        if bool((gids == -1).all()):
            return images, targets, aux, masks
        perm = self._perm(gids)
        alpha = self.mix_config.get("ALPHA", 1.0)
        lam = float(inj["lam"]) if inj else float(torch.distributions.beta.Beta(alpha, alpha).sample())
        if self.minmax is not None:
            lam = self.minmax[0] + (self.minmax[1] - self.minmax[0]) * lam
        B, Cc, H, W = images.shape
        bbx1, bby1, bbx2, bby2 = inj["box"] if inj else rand_bbox((1, Cc, H, W), lam)
        lam_adj = 1.0 - ((bbx2 - bbx1) * (bby2 - bby1) / (H * W))
        valid = gids != -1
        # the reference cuts images[:, :, bbx1:bbx2, bby1:bby2]: "x" runs over dim 2 (rows), "y" over dim 3 (columns)
        mixed_images = _mix_rows(images, perm, 0.0, 1, valid, (int(bbx1), int(bbx2), int(bby1), int(bby2)), (H, W))
        mixed_targets = {k: _mix_rows(v, perm, lam_adj, 2, valid) for k, v in targets.items()}
        mixed_aux, mixed_masks = self._mix_meta(aux, masks, perm, inj["pick"].to(aux.device) if inj else None)
        return mixed_images, mixed_targets, mixed_aux, mixed_masks


# --- scheduled metadata masking (h5data/h5dataloader.py:709-940, ops_schedule.py:450-650) ---------------------------------------


def _cfg_get(node, name, default=None):
    """attribute or mapping entry of a config node (yacs CfgNode, dict or a plain namespace)"""
    if node is None:
        return default
    if isinstance(node, dict):
        return node.get(name, default)
    return getattr(node, name, default)


def partial_mask_tables(component_names, whitelist, weights=None) -> Tuple[List[int], List[float]]:
    """(bitmask per combination, fp32 cumulative pick thresholds) of a partial-masking whitelist, by the rules of
    ops_schedule.py:628-650 and _apply_partial_mask: the weights count only when there is one per combination (else the pick is
    uniform), component names that are not in the bounds map are dropped, an empty whitelist gives empty tables (no masking).  The
    last threshold is forced to 1 so that every draw of [0, 1) picks a combination."""
    names = list(component_names)
    combos = [list(c) for c in (whitelist or [])]
    if not combos:
        return [], []
    w = [float(v) for v in weights] if weights and len(weights) == len(combos) else [1.0] * len(combos)
    if any(v < 0 or v != v for v in w):
        raise ValueError(f"partial meta-mask weights must be non-negative (got {w})")
    total = math.fsum(w)
    if not total > 0:
        raise ValueError("partial meta-mask weights sum to 0")
    bits = [sum(1 << names.index(n) for n in set(c) if n in names) for c in combos]
    acc, thr = 0.0, []
    for v in w:
        acc += v
        thr.append(float(torch.tensor(min(acc / total, 1.0), dtype=torch.float32)))
    thr[-1] = 1.0
    return bits, thr


def _meta_mask_launch(aux, mask_u8, out_aux, out_mask, B, D, bounds_dev, ncomp, *, tables=None, draws=None, combo_idx=None, p_full=0.0, p_partial=0.0,
                      partial_on=False, row_bits=0, row_full=False, counts=None, row_combo=None):
    a = L.MetaMaskArgs()
    a.aux = aux.data_ptr() if aux is not None else None
    a.mask = mask_u8.data_ptr() if mask_u8 is not None else None
    a.out_aux = out_aux.data_ptr() if out_aux is not None else None
    a.out_mask = out_mask.data_ptr() if out_mask is not None else None
    a.B, a.D, a.ncomp = B, D, ncomp
    a.bounds = bounds_dev.data_ptr() if ncomp else None
    if tables is not None and tables[0] is not None:
        a.ncombo, a.combo_bits, a.combo_thr = tables[0].numel(), tables[0].data_ptr(), tables[1].data_ptr()
    a.draws = draws.data_ptr() if draws is not None else None
    a.combo_idx = combo_idx.data_ptr() if combo_idx is not None else None
    a.p_full, a.p_partial, a.partial_on = float(p_full), float(p_partial), int(bool(partial_on))
    a.row_bits, a.row_full = int(row_bits), int(bool(row_full))
    a.counts = counts.data_ptr() if counts is not None else None
    a.row_combo = row_combo.data_ptr() if row_combo is not None else None
    L.check(L.lib().lnx_meta_mask(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "lnx_meta_mask")


def _check_bounds(bounds, D):
    for s, e in bounds:
        if not 0 <= s <= e <= D:
            raise ValueError(f"metadata component bounds ({s}, {e}) lie outside [0, {D}]")


def _as_bytes(masks: torch.Tensor) -> torch.Tensor:
    m = masks.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m.to(torch.uint8)


def _need_gpu(t: torch.Tensor):
    if not t.is_cuda:
        raise L.LnxError("linnaeus_amd.collate runs on the HIP kernels only: move the batch to the GPU first")


class GPUMetaMasking:
    """The training-time metadata masking of H5DataLoader.collate_fn (h5data/h5dataloader.py:709-940) on a device batch: rows with
    u_full < p_full lose all of aux_info and their validity mask; of the others, rows with u_partial < p_partial lose the components of
    one whitelist combination.  One `torch.rand(3, B)` and one lnx_meta_mask launch, no host read; the inputs are not modified.

    `meta_chunk_bounds_map` is the reference's {component: (start, end)}; `ops_schedule` is duck-typed (the getters of
    ops_schedule.py:450-626 and `meta_cfg.PARTIAL.WHITELIST / WEIGHTS`)."""

    def __init__(self, meta_chunk_bounds_map, ops_schedule=None, whitelist=None, weights=None):
        self.components = list(meta_chunk_bounds_map.keys())
        self.bounds = [(int(s), int(e)) for s, e in meta_chunk_bounds_map.values()]
        if len(self.components) > L.META_MASK_MAX_COMPONENTS:
            raise ValueError(f"{len(self.components)} metadata components: the masking kernel takes at most {L.META_MASK_MAX_COMPONENTS}")
        self.ops_schedule = ops_schedule
        pm = _cfg_get(_cfg_get(ops_schedule, "meta_cfg"), "PARTIAL")
        if whitelist is None:
            whitelist = _cfg_get(pm, "WHITELIST")
        if weights is None:
            weights = _cfg_get(pm, "WEIGHTS")
        self.combo_bits, self.combo_thr = partial_mask_tables(self.components, whitelist, weights)
        self._dev = {}
        self._checked_D = set()
        self._inject = None  # tests: dict(draws= [3, B] fp32, combo_idx= [B] int or None) recorded from the reference run
        self.last_counts = None
        self.last_row_combo = None
        self.record_row_combo = False  # tests: keep the combination each row took in last_row_combo

    def _tables(self, device):
        t = self._dev.get(str(device))
        if t is None:
            bd = torch.tensor([v for se in self.bounds for v in se], dtype=torch.int32, device=device)
            if self.combo_bits:
                cb = torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in self.combo_bits], dtype=torch.int32, device=device)
                ct = torch.tensor(self.combo_thr, dtype=torch.float32, device=device)
            else:
                cb = ct = None
            t = self._dev[str(device)] = (bd, cb, ct)
        return t

    def _shape(self, t):
        B, D = t.shape
        if D not in self._checked_D:
            _check_bounds(self.bounds, D)
            self._checked_D.add(D)
        return B, D

    def probabilities(self, step=None):
        """(p_full, partial_enabled, p_partial) as collate_fn reads them from the schedule (h5dataloader.py:647-665, 800-810)"""
        s = self.ops_schedule
        if s is None:
            raise ValueError("GPUMetaMasking: no ops_schedule, pass p_full / partial_enabled / p_partial")
        if step is None:
            tp = getattr(s, "training_progress", None)
            step = tp.global_step if tp is not None else 0
        p_full = s.get_meta_mask_prob_by_iteration(step) if hasattr(s, "get_meta_mask_prob_by_iteration") else s.get_meta_mask_prob(step)
        partial = bool(s.get_partial_mask_enabled())
        p_partial = s.get_partial_meta_mask_prob() if hasattr(s, "get_partial_meta_mask_prob") else 1.0
        return float(p_full), partial, float(p_partial)

    def __call__(self, aux, masks, step=None, *, p_full=None, partial_enabled=None, p_partial=None, generator=None):
        _need_gpu(aux)
        _need_gpu(masks)
        if None in (p_full, partial_enabled, p_partial):
            sp = self.probabilities(step)
            p_full = sp[0] if p_full is None else p_full
            partial_enabled = sp[1] if partial_enabled is None else partial_enabled
            p_partial = sp[2] if p_partial is None else p_partial
        B, D = self._shape(aux)
        bd, cb, ct = self._tables(aux.device)
        inj = self._inject
        combo_idx = None
        if inj is not None:
            draws = inj["draws"].to(device=aux.device, dtype=torch.float32).contiguous()
            if inj.get("combo_idx") is not None:
                combo_idx = inj["combo_idx"].to(device=aux.device, dtype=torch.int32).contiguous()
        else:
            draws = torch.rand(3, B, device=aux.device, generator=generator)
        if tuple(draws.shape) != (3, B):
            raise ValueError(f"draws must be [3, {B}], got {tuple(draws.shape)}")
        af = aux.float().contiguous()
        mk = _as_bytes(masks)
        oa, om = torch.empty_like(af), torch.empty_like(mk)
        counts = torch.zeros(2 + len(self.bounds), dtype=torch.int32, device=aux.device)
        rc = torch.empty(B, dtype=torch.int32, device=aux.device) if self.record_row_combo else None
        _meta_mask_launch(af, mk, oa, om, B, D, bd, len(self.bounds), tables=(cb, ct), draws=draws, combo_idx=combo_idx, p_full=p_full,
                          p_partial=p_partial, partial_on=partial_enabled, counts=counts, row_combo=rc)
        self.last_counts, self.last_row_combo = counts, rc
        return oa.to(aux.dtype), (om.view(torch.bool) if masks.dtype == torch.bool else om.to(masks.dtype))

    def counts_of(self, masks) -> torch.Tensor:
        """device int32[ncomp]: per component, the rows whose mask is all-true over it (one launch, nothing is masked)"""
        _need_gpu(masks)
        B, D = self._shape(masks)
        counts = torch.zeros(2 + len(self.bounds), dtype=torch.int32, device=masks.device)
        _meta_mask_launch(None, _as_bytes(masks), None, None, B, D, self._tables(masks.device)[0], len(self.bounds), counts=counts)
        return counts[2:]

    def stats(self, masks) -> torch.Tensor:
        """device float64[ncomp]: `actual_meta_stats` of h5dataloader.py:1740-1801, (valid rows / B) * 100 per component"""
        return self.counts_of(masks).to(torch.float64) / masks.shape[0] * 100.0

    def stats_dict(self, masks=None, *, stats=None) -> Dict[str, float]:
        """{component: valid percentage}, the reference's `actual_meta_stats`: the single read-back, of `stats` (what stats() or
        GPUTrainCollate returned) or of the statistics of `masks`"""
        st = self.stats(masks) if stats is None else stats
        return dict(zip(self.components, st.cpu().tolist()))


def mask_meta_components(aux, bounds_map, components=None):
    """The evaluation-time masking of validation.py on a device batch, as a new tensor from one launch: `components=None` zeroes all
    of aux_info (validate_one_pass(mask_meta=True), :174-175), a list zeroes the columns of those components
    (validate_with_partial_mask, :428-489)."""
    _need_gpu(aux)
    names = list(bounds_map.keys())
    if len(names) > L.META_MASK_MAX_COMPONENTS:
        raise ValueError(f"{len(names)} metadata components: the masking kernel takes at most {L.META_MASK_MAX_COMPONENTS}")
    bounds = [(int(s), int(e)) for s, e in bounds_map.values()]
    B, D = aux.shape
    _check_bounds(bounds, D)
    bits = 0
    for c in components or []:
        if c not in names:
            raise KeyError(f"unknown metadata component {c!r} (known: {names})")
        bits |= 1 << names.index(c)
    af = aux.float().contiguous()
    out = torch.empty_like(af)
    bd = torch.tensor([v for se in bounds for v in se], dtype=torch.int32, device=aux.device)
    _meta_mask_launch(af, None, out, None, B, D, bd, len(bounds), row_bits=bits, row_full=components is None)
    return out.to(aux.dtype)


def _check_combos(combos, names=None) -> list:
    """A list of variants: () = aux_info as it is, None = all of it zeroed, else the component names whose columns are zeroed."""
    if isinstance(combos, str) or combos is None:
        raise TypeError("combos must be a sequence of variants: (), None or a list of component names each")
    out = []
    for c in combos:
        if c is None:
            out.append(None)
            continue
        if isinstance(c, str):
            raise TypeError(f"a combo is a list of component names, not the string {c!r}")
        c = tuple(c)
        for n in c:
            if not isinstance(n, str):
                raise TypeError(f"component names are strings, got {n!r}")
            if names is not None and n not in names:
                raise KeyError(f"unknown metadata component {n!r} (known: {list(names)})")
        out.append(c)
    if not out:
        raise ValueError("no metadata variants given")
    return out


def variant_phase_names(combos) -> List[str]:
    """The reference's phase name of each variant: `val` for () (validation.py:84), `val_mask_meta` for None (all of aux_info
    zeroed, :84,174-175), `val_mask_<A_B>` for the components A, B (main.py:2207)."""
    names = ["val_mask_meta" if c is None else ("val_mask_" + "_".join(c) if c else "val") for c in _check_combos(combos)]
    if len(set(names)) != len(names):
        raise ValueError(f"metadata variants repeat a phase: {names}")
    return names


def meta_variants(aux, bounds_map, combos):
    """[K, B, W]: aux_info as each of the K validation passes of the reference sees it (validate_one_pass, validation.py:174-175;
    validate_with_partial_mask, :428-489), for `mFormerV1.forward_meta_variants`.  A combo is a list of component names; () means
    unmasked and None all of aux_info zeroed.  One mask_meta_components launch per masked variant; `aux` is not modified."""
    combos = _check_combos(combos, list(bounds_map.keys()))
    if aux.dim() != 2:
        raise ValueError(f"aux must be [B, W], got {tuple(aux.shape)}")
    _need_gpu(aux)
    out = torch.empty((len(combos),) + tuple(aux.shape), dtype=aux.dtype, device=aux.device)
    for k, c in enumerate(combos):
        out[k].copy_(aux if c == () else mask_meta_components(aux, bounds_map, None if c is None else list(c)))
    return out


class GPUTrainCollate:
    """The training half of H5DataLoader.collate_fn (h5data/h5dataloader.py:642-1801) on a device batch
    `(images, targets, aux, masks, group_ids)`, in the reference's order: metadata masking, the mixing decision against
    get_mixup_prob (a host draw), should_use_cutmix(), GPUSelectiveCutMix / GPUSelectiveMixup, then the component statistics of the
    final masks.  Returns `(images, targets, aux, masks, stats_device)`; `masker.stats_dict(stats=stats_device)` is the read-back.
    `mixup` / `cutmix` take ready mixers (else they are built from config.SCHEDULE.MIX); PROB is set to the scheduled probability
    on every batch, as the reference builds its mixer per batch."""

    def __init__(self, ops_schedule, meta_chunk_bounds_map, mixup=None, cutmix=None):
        self.ops_schedule = ops_schedule
        self.masker = GPUMetaMasking(meta_chunk_bounds_map, ops_schedule)
        self.config = getattr(ops_schedule, "config", None)
        mix = _cfg_get(_cfg_get(self.config, "SCHEDULE"), "MIX")
        self.exclude_null_samples = bool(_cfg_get(mix, "EXCLUDE_NULL_SAMPLES", False))
        self.null_task_keys = _cfg_get(mix, "NULL_TASK_KEYS")
        bounds_list = [list(b) for b in self.masker.bounds]
        if mixup is None:
            mixup = GPUSelectiveMixup({"PROB": 0.0, "ALPHA": _cfg_get(_cfg_get(mix, "MIXUP"), "ALPHA", 1.0), "meta_chunk_bounds_list": bounds_list}, config=self.config)
        if cutmix is None:
            cm = _cfg_get(mix, "CUTMIX")
            cfg = {"PROB": 0.0, "ALPHA": _cfg_get(cm, "ALPHA", 1.0), "meta_chunk_bounds_list": bounds_list}
            if _cfg_get(cm, "MINMAX") is not None:
                cfg["MINMAX"] = _cfg_get(cm, "MINMAX")
            cutmix = GPUSelectiveCutMix(cfg, config=self.config)
        self.mixup, self.cutmix = mixup, cutmix
        self.last_mixed = None  # None, "mixup" or "cutmix": what the last batch went through

    def _step(self):
        tp = getattr(self.ops_schedule, "training_progress", None)
        return tp.global_step if tp is not None else 0

    def _mixes(self):
        sampler = _cfg_get(_cfg_get(self.config, "DATA"), "SAMPLER")
        return sampler is None or str(_cfg_get(sampler, "TYPE", "")).lower() == "grouped"

    def __call__(self, batch, step=None, generator=None):
        images, targets, aux, masks, gids = batch
        s = self.ops_schedule
        step = self._step() if step is None else step
        aux, masks = self.masker(aux, masks, step, generator=generator)
        self.last_mixed = None
        if self._mixes():
            prob = s.get_mixup_prob_by_iteration(step) if hasattr(s, "get_mixup_prob_by_iteration") else s.get_mixup_prob(step)
            if torch.rand(1).item() < prob:
                use_cutmix = bool(s.should_use_cutmix()) if hasattr(s, "should_use_cutmix") else False
                mixer = self.cutmix if use_cutmix else self.mixup
                mixer.mix_config["PROB"] = prob
                keys = self.null_task_keys if self.null_task_keys is not None else list(targets.keys())
                images, targets, aux, masks = mixer((images, targets, aux, masks, gids), exclude_null_samples=self.exclude_null_samples, null_task_keys=keys)
                self.last_mixed = "cutmix" if use_cutmix else "mixup"
        return images, targets, aux, masks, self.masker.stats(masks)
