"""Validation metrics accumulated on the device: one HIP launch per batch, no host synchronisation until compute().

DeviceMetrics does the per-batch bookkeeping of the reference's MetricsTracker._update_phase_batch (utils/metrics/tracker.py:609-937:
chain and partial chain accuracy, per-task acc1 / acc3 / loss, the null / non-null split, per-subset acc1) with lnx_metrics_update,
which only adds to two device tables.  compute() reads them back once; flush_into() adds them to the accumulators the
reference's tracker finalises from, so a validation loop swaps `update_val_metrics` for `update` and flushes once per phase.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import _lib as L
from . import ops


def _rank(task_key: str) -> int:
    return int(task_key.split("_L")[-1])


class DeviceMetrics:
    def __init__(self, task_keys: Sequence[str], num_classes, null_tracking_tasks: Sequence[str] = (), subset_bins: Optional[Dict[str, int]] = None):
        """task_keys: `..._L<n>` keys (sorted here by <n>, as the tracker does); num_classes: {task: C} or a sequence parallel to
        task_keys; null_tracking_tasks: the tasks whose null / non-null figures compute() and flush_into() report; subset_bins:
        {subset type: number of ids}, at most two types."""
        keys = list(task_keys)
        if not isinstance(num_classes, dict):
            num_classes = dict(zip(keys, num_classes))
        self.task_keys = sorted(keys, key=_rank)
        if not 1 <= len(self.task_keys) <= L.METRICS_MAX_TASKS:
            raise L.LnxError(f"DeviceMetrics: {len(self.task_keys)} tasks (1..{L.METRICS_MAX_TASKS})")
        self.num_classes = [int(num_classes[t]) for t in self.task_keys]
        unknown = [t for t in null_tracking_tasks if t not in self.task_keys]
        if unknown:
            raise L.LnxError(f"DeviceMetrics: null tracking for unknown tasks {unknown}")
        self.null_tracking_tasks = [t for t in self.task_keys if t in set(null_tracking_tasks)]
        self.subset_bins = dict(subset_bins or {})
        if len(self.subset_bins) > 2 or any(int(n) < 1 for n in self.subset_bins.values()):
            raise L.LnxError("DeviceMetrics: at most two subset types, each with at least one bin")
        self._subset_types = list(self.subset_bins)
        self._n_bins = [int(self.subset_bins[s]) for s in self._subset_types]
        nb = self._n_bins + [0, 0]
        self._n_counts, self._n_sums = ops.metrics_table_sizes(len(self.task_keys), nb[0], nb[1])
        self.counts: Optional[torch.Tensor] = None  # int64 [n_counts] / float64 [n_sums] on the device of the first update
        self.sums: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------------------------------------------------------
    def reset(self) -> None:
        if self.counts is not None:
            self.counts.zero_()
            self.sums.zero_()

    def update(self, outputs, targets, per_sample_losses=None, subset_ids=None) -> None:
        """outputs: {task: [B, C] logits, fp32 or bf16, contiguous or padded row views}; targets: {task: int [B] class indices or
        [B, C] one-hot / soft rows}; per_sample_losses: {task: [B]} (any subset of the tasks); subset_ids: {subset type: int [B]}.
        Enqueues a few torch casts where the inputs need them and ONE lnx_metrics_update; never synchronises."""
        first = outputs[self.task_keys[0]]
        if self.counts is None:
            self.counts = torch.zeros(self._n_counts, dtype=torch.int64, device=first.device)
            self.sums = torch.zeros(self._n_sums, dtype=torch.float64, device=first.device)
        logits, tgts, nulls, losses = [], [], [], []
        for t, C_ in zip(self.task_keys, self.num_classes):
            x, tg = outputs[t], targets[t]
            if isinstance(x, dict):
                raise L.LnxError(f"DeviceMetrics: dict-valued head output for {t} is not supported")
            if x.dtype != first.dtype or x.dtype not in (torch.float32, torch.bfloat16):
                x = x.float() if first.dtype == torch.float32 else x.to(first.dtype)
            if x.shape[1] > 1 and x.stride(1) != 1:
                x = x.contiguous()
            if x.shape[1] < C_:
                raise L.LnxError(f"DeviceMetrics: {t} has {x.shape[1]} logit columns, {C_} classes")
            nul = None
            if tg.dim() > 1:  # tracker.py:796-803: class = argmax, null = the first column above 0.5
                nul = (tg[:, 0] > 0.5).to(torch.uint8)
                tg = tg.argmax(1)
            tg = tg.to(device=x.device, dtype=torch.int64, non_blocking=True).contiguous()
            ls = per_sample_losses.get(t) if per_sample_losses is not None else None
            if ls is not None:
                ls = ls.detach().to(torch.float32).contiguous()
            logits.append(x.detach())
            tgts.append(tg)
            nulls.append(nul)
            losses.append(ls)
        ids = [None, None]
        for s, name in enumerate(self._subset_types):
            if subset_ids is not None and subset_ids.get(name) is not None:
                ids[s] = subset_ids[name].to(device=first.device, dtype=torch.int64, non_blocking=True).contiguous()
        nb = [n if i is not None else 0 for i, n in zip(ids, self._n_bins + [0, 0])]
        if ids[0] is None and ids[1] is not None and self._n_bins[0]:  # type 1's bins sit behind type 0's: keep the layout
            raise L.LnxError("DeviceMetrics: subset ids of the second type need those of the first")
        ops.metrics_update(logits, tgts, self.counts, self.sums, num_classes=self.num_classes, is_null=nulls, losses=losses, subset_ids=ids, n_bins=nb)

    # ------------------------------------------------------------------------------------------------------------------
    def _tables(self):
        """Both tables on the host: one all-reduce of each under an initialised torch.distributed, then one device-to-host copy."""
        if self.counts is None:
            return [0] * self._n_counts, [0.0] * self._n_sums
        counts, sums = self.counts, self.sums
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            counts, sums = counts.clone(), sums.clone()
            dist.all_reduce(counts)
            dist.all_reduce(sums)
        # one copy: the sums travel as their bit patterns behind the counters
        both = torch.cat([counts, sums.view(torch.int64)]).cpu()
        return both[: self._n_counts].tolist(), both[self._n_counts:].view(torch.float64).tolist()

    def _raw(self) -> dict:
        counts, sums = self._tables()
        T = len(self.task_keys)
        raw = {"chain_correct": counts[L.METRICS_CHAIN_CORRECT], "chain_total": counts[L.METRICS_CHAIN_N],
               "partial_chain_correct": counts[L.METRICS_PARTIAL_CORRECT], "partial_chain_total": counts[L.METRICS_PARTIAL_N], "tasks": {}, "subsets": {}}
        names = ("n", "correct1", "correct3", "null_n", "null_correct1", "non_null_n", "non_null_correct1", "loss_n")
        for i, t in enumerate(self.task_keys):
            d = {k: counts[L.metrics_task(i) + j] for j, k in enumerate(names)}
            s0 = L.METRICS_SUM_STRIDE * i
            d.update(loss_sum=sums[s0 + L.METRICS_SUM_LOSS], null_loss_sum=sums[s0 + L.METRICS_SUM_NULL_LOSS], non_null_loss_sum=sums[s0 + L.METRICS_SUM_NONNULL_LOSS])
            raw["tasks"][t] = d
        nb0 = self._n_bins[0] if self._n_bins else 0
        for s, name in enumerate(self._subset_types):
            base, nb = L.metrics_subset(T, nb0, s), self._n_bins[s]
            per_task = {}
            for i, t in enumerate(self.task_keys):
                seg = counts[base + 2 * i * nb: base + 2 * (i + 1) * nb]
                per_task[t] = {"n": seg[0::2], "correct1": seg[1::2]}
            raw["subsets"][name] = {"out_of_range": counts[L.METRICS_SUBSET_OOR + s], "tasks": per_task}
        return raw

    def compute(self) -> dict:
        """The tracker's metric names -> floats, plus "subsets" ({type: {task: {id: acc1}}}, ids seen at least once) and "counts"
        (every raw counter).  Zero denominators: 1.0 for the two chain figures (chain_accuracy.py:166,344), the key is absent elsewhere."""
        raw = self._raw()
        out = {"chain_accuracy": raw["chain_correct"] / raw["chain_total"] if raw["chain_total"] > 0 else 1.0,
               "partial_chain_accuracy": raw["partial_chain_correct"] / raw["partial_chain_total"] if raw["partial_chain_total"] > 0 else 1.0}
        for t, d in raw["tasks"].items():
            if d["n"] > 0:
                out[f"acc1_{t}"] = d["correct1"] / d["n"]
                out[f"acc3_{t}"] = d["correct3"] / d["n"]
            if d["loss_n"] > 0:
                out[f"loss_{t}"] = d["loss_sum"] / d["loss_n"]
            if t in self.null_tracking_tasks:
                for kind in ("null", "non_null"):
                    if d[f"{kind}_n"] > 0:
                        out[f"{kind}_acc1_{t}"] = d[f"{kind}_correct1"] / d[f"{kind}_n"]
                        if d["loss_n"] > 0:
                            out[f"{kind}_loss_{t}"] = d[f"{kind}_loss_sum"] / d[f"{kind}_n"]
        out["subsets"] = {name: {t: {i: c / n for i, (n, c) in enumerate(zip(v["n"], v["correct1"])) if n > 0} for t, v in sub["tasks"].items()}
                          for name, sub in raw["subsets"].items()}
        out["counts"] = raw
        return out

    def flush_into(self, tracker, phase: str) -> None:
        """Add everything accumulated since the last reset() to the reference tracker's accumulators for `phase` (the ones
        finalize_val_phase reads), then reset().  The tracker is duck-typed: plain attributes holding dicts."""
        raw = self._raw()
        tracker.chain_correct[phase] += raw["chain_correct"]
        tracker.chain_total[phase] += raw["chain_total"]
        tracker.partial_chain_correct[phase] += raw["partial_chain_correct"]
        tracker.partial_chain_total[phase] += raw["partial_chain_total"]
        for t, d in raw["tasks"].items():
            sums, cnts = tracker.partial_task_sums[phase][t], tracker.partial_task_counts[phase][t]
            sums["acc1"] += d["correct1"]
            cnts["acc1"] += d["n"]
            sums["acc3"] += d["correct3"]
            cnts["acc3"] += d["n"]
            if d["loss_n"] > 0:
                sums["loss"] += d["loss_sum"]
                cnts["loss"] += d["loss_n"]
            if t not in self.null_tracking_tasks or d["loss_n"] == 0:  # (the tracker splits only where it has the per-sample losses: tracker.py:772)
                continue
            for kind, s_tab, c_tab in (("null", tracker.partial_null_sums, tracker.partial_null_counts),
                                       ("non_null", tracker.partial_non_null_sums, tracker.partial_non_null_counts)):
                if d[f"{kind}_n"] > 0:
                    s_tab[phase][t]["acc1"] += d[f"{kind}_correct1"]
                    c_tab[phase][t]["acc1"] += d[f"{kind}_n"]
                    s_tab[phase][t]["loss"] += d[f"{kind}_loss_sum"]
                    c_tab[phase][t]["loss"] += d[f"{kind}_n"]
        self.reset()


class MetaVariantEvaluator:
    """The reference's validation passes over the same images with different metadata (`val`, `val_mask_meta`, `val_mask_<A_B>`:
    validation.py:84,174-175,341-617, main.py:2207) from ONE pass over the data: per batch one `forward_meta_variants` (one trunk, K
    token-stage passes) and one DeviceMetrics.update per variant."""

    def __init__(self, model, bounds_map, combos, task_keys: Sequence[str], num_classes, null_tracking_tasks: Sequence[str] = (),
                 subset_bins: Optional[Dict[str, int]] = None, per_sample_loss=None):
        """combos: the variants (`collate.meta_variants`: () unmasked, None all of aux_info zeroed, else component names);
        per_sample_loss: callable (outputs, targets) -> {task: [B]}, called once per variant.  The other arguments are DeviceMetrics'."""
        from .collate import _check_combos, variant_phase_names

        self.model = model
        self.bounds_map = dict(bounds_map)
        self.combos = _check_combos(combos, list(self.bounds_map.keys()))
        self.phases = variant_phase_names(self.combos)
        self.per_sample_loss = per_sample_loss
        self.metrics = {ph: DeviceMetrics(task_keys, num_classes, null_tracking_tasks, subset_bins) for ph in self.phases}

    def reset(self) -> None:
        for m in self.metrics.values():
            m.reset()

    def update(self, images, aux, targets, subset_ids=None) -> None:
        """Enqueues the masking launches, the forward and its K - 1 tails, and per variant the loss (if any) and one metrics launch;
        never synchronises."""
        from .collate import meta_variants

        module = getattr(self.model, "module", self.model)  # (ddp.DataParallel: the wrapped model)
        was_training = module.training
        module.eval()
        try:
            with torch.no_grad():
                outs = module.forward_meta_variants(images, meta_variants(aux, self.bounds_map, self.combos))
                for ph, out in zip(self.phases, outs):
                    losses = self.per_sample_loss(out, targets) if self.per_sample_loss is not None else None
                    self.metrics[ph].update(out, targets, per_sample_losses=losses, subset_ids=subset_ids)
        finally:
            module.train(was_training)

    def compute(self) -> dict:
        """{phase: DeviceMetrics.compute()}"""
        return {ph: m.compute() for ph, m in self.metrics.items()}

    def flush_into(self, tracker) -> None:
        """DeviceMetrics.flush_into for every phase, under the reference's phase names."""
        for ph, m in self.metrics.items():
            m.flush_into(tracker, ph)
