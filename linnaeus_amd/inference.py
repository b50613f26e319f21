"""Predictions on the device: one HIP launch per batch from {task: logits} to the final top-k lists, no host synchronisation.

DevicePredictor does what the reference's LinnaeusInferenceHandler.predict does after the forward (inference/handler.py:186-228: per
sample and task softmax, topk and two .item() per kept entry) and then enforce_hierarchical_consistency
(inference/postprocessing.py:14-171, a Python walk of the taxonomy tree per sample) with lnx_predict, which reads every logit once and
writes four device tensors.  to_results() copies them to the host once and returns plain Python lists.

What differs from the reference: probabilities are an fp32 softmax whatever the logits' dtype (the reference runs softmax in the
autocast dtype); equal values are ordered by ascending class index, NaN first; results are tuples, not `typus` objects; image and
metadata preprocessing and artifact loading are the caller's.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from . import _lib as L
from . import ops


def _rank(task_key: str) -> int:
    return int(task_key.split("_L")[-1])


class DevicePredictor:
    def __init__(self, task_keys: Sequence[str], num_classes, taxonomy_tree=None, parent_index: Optional[Dict[str, torch.Tensor]] = None,
                 null_index=0, top_k: int = 5, consistency: bool = True, idx_to_taxon_id=None):
        """task_keys: `..._L<n>` keys (sorted here by <n>: finest first, as DATA.TASK_KEYS_H5); num_classes: {task: C} or a sequence
        parallel to task_keys.  The parent tables (class -> class of the next coarser task) come from ONE of
          taxonomy_tree   a reference TaxonomyTree or anything with get_parent((task, idx)) -> (task, idx) | None,
                          or a module / mapping holding the `hmatrix_{parent}_{child}` buffers of a hierarchical head ([n_parent, n_child]
                          0/1 membership: the parent is the column's arg-max, -1 for an all-zero column);
          parent_index    {task: integer [C]} for every task but the coarsest (-1 = no parent).
        null_index: an int for every task, or {task: int | None} (None: the task has no null class and is never nullified);
        top_k: the default list length (1..16); idx_to_taxon_id: {task: {class index: id} | integer [C]} for any subset of the tasks."""
        keys = list(task_keys)
        if not isinstance(num_classes, dict):
            num_classes = dict(zip(keys, num_classes))
        self.task_keys = sorted(keys, key=_rank)
        T = len(self.task_keys)
        if not 1 <= T <= L.METRICS_MAX_TASKS:
            raise L.LnxError(f"DevicePredictor: {T} tasks (1..{L.METRICS_MAX_TASKS})")
        self.num_classes = [int(num_classes[t]) for t in self.task_keys]
        self.top_k = self._check_k(top_k)
        self.consistency = bool(consistency)
        if isinstance(null_index, dict):
            unknown = [t for t in null_index if t not in self.task_keys]
            if unknown:
                raise L.LnxError(f"DevicePredictor: null index for unknown tasks {unknown}")
            self.null_index = [null_index.get(t, 0) for t in self.task_keys]
        else:
            self.null_index = [null_index] * T
        for t, n, c in zip(self.task_keys, self.null_index, self.num_classes):
            if n is not None and not 0 <= int(n) < c:
                raise L.LnxError(f"DevicePredictor: null index {n} of {t} is outside [0, {c})")
        self.null_index = [None if n is None else int(n) for n in self.null_index]
        if taxonomy_tree is not None and parent_index is not None:
            raise L.LnxError("DevicePredictor: give taxonomy_tree or parent_index, not both")
        self.parent_index: List[Optional[torch.Tensor]] = self._parent_tables(taxonomy_tree, parent_index)  # int32 [C] on the host
        if self.consistency and any(p is None for p in self.parent_index[:-1]):
            raise L.LnxError("DevicePredictor: consistency needs the parent table of every task but the coarsest")
        self.id_maps: List[Optional[torch.Tensor]] = [None] * T  # int64 [C] on the host
        for t, m in (idx_to_taxon_id or {}).items():
            if t not in self.task_keys:
                raise L.LnxError(f"DevicePredictor: id map for unknown task {t}")
            i = self.task_keys.index(t)
            if isinstance(m, dict):
                m = [m[j] for j in range(self.num_classes[i])]
            m = torch.as_tensor(m, dtype=torch.int64).reshape(-1).contiguous()
            if m.numel() != self.num_classes[i]:
                raise L.LnxError(f"DevicePredictor: id map of {t} has {m.numel()} entries, {self.num_classes[i]} classes")
            self.id_maps[i] = m
        self._device = None
        self._dev_parents = self._dev_ids = None

    # ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_k(k) -> int:
        k = int(k)
        if not 1 <= k <= L.PREDICT_MAX_K:
            raise L.LnxError(f"DevicePredictor: top_k={k} (1..{L.PREDICT_MAX_K})")
        return k

    def _parent_tables(self, tree, explicit):
        T = len(self.task_keys)
        tabs: List[Optional[torch.Tensor]] = [None] * T
        for i in range(T - 1):
            child, parent, C_ = self.task_keys[i], self.task_keys[i + 1], self.num_classes[i]
            tab = None
            if explicit is not None:
                if child in explicit:
                    tab = torch.as_tensor(explicit[child]).detach().cpu().to(torch.int64).reshape(-1)
            elif tree is not None and hasattr(tree, "get_parent"):
                tab = torch.full((C_,), -1, dtype=torch.int64)
                for c in range(C_):
                    node = tree.get_parent((child, c))
                    if node is not None and node[0] == parent:
                        tab[c] = int(node[1])
            elif tree is not None:
                name = f"hmatrix_{parent}_{child}"
                m = tree.get(name) if isinstance(tree, dict) else getattr(tree, name, None)
                if m is not None:
                    m = m.detach().cpu()
                    if tuple(m.shape) != (self.num_classes[i + 1], C_):
                        raise L.LnxError(f"DevicePredictor: {name} is {tuple(m.shape)}, expected {(self.num_classes[i + 1], C_)}")
                    tab = torch.where(m.ne(0).any(0), m.argmax(0), torch.full((C_,), -1, dtype=torch.int64))
            if tab is None:
                continue
            if tab.numel() != C_ or int(tab.max()) >= self.num_classes[i + 1] or int(tab.min()) < -1:
                raise L.LnxError(f"DevicePredictor: parent table of {child} must hold {C_} entries in [-1, {self.num_classes[i + 1]})")
            tabs[i] = tab.to(torch.int32).contiguous()
        return tabs

    def _tables_on(self, device):
        if self._device != device:  # built once, kept on the device
            self._dev_parents = [None if p is None else p.to(device) for p in self.parent_index]
            self._dev_ids = [None if m is None else m.to(device) for m in self.id_maps]
            self._device = device
        return self._dev_parents, self._dev_ids

    def _k_args(self, top_k, B: int, device):
        """top_k -> (K of the launch, int32 [B] on the device or None)"""
        if top_k is None:
            return self.top_k, None
        if isinstance(top_k, int):
            return self._check_k(top_k), None
        if isinstance(top_k, torch.Tensor):
            if top_k.dim() == 0:
                return self._check_k(top_k.item()), None
            if top_k.shape != (B,):
                raise L.LnxError(f"DevicePredictor: per-sample top_k must be [B = {B}], got {tuple(top_k.shape)}")
            # a device tensor is taken as it is (no read-back): the launch keeps K = 16 rows and clamps each value into [1, 16]
            K = L.PREDICT_MAX_K if top_k.is_cuda else self._check_k(max(self._check_k(v) for v in top_k.tolist()))
            return K, top_k.to(device=device, dtype=torch.int32, non_blocking=True).contiguous()
        ks = [self._check_k(self.top_k if v is None else v) for v in top_k]  # the handler's per_sample_overrides: None = the default
        if len(ks) != B:
            raise L.LnxError(f"DevicePredictor: {len(ks)} per-sample top_k values for a batch of {B}")
        return max(ks), torch.tensor(ks, dtype=torch.int32).to(device, non_blocking=True)

    # ------------------------------------------------------------------------------------------------------------------
    def predict_logits(self, outputs, top_k=None) -> Dict[str, torch.Tensor]:
        """outputs: {task: [B, C] logits, fp32 or bf16, contiguous or padded row views}, taken as they come (no copies); top_k: None
        (the default), an int, or per-sample values ([B] tensor or list).  Enqueues ONE lnx_predict and never synchronises.  Returns
        device tensors {"ids": int64 [B, T, K], "probs": fp32 [B, T, K], "count": int32 [B, T], "flags": int32 [B, T]}, tasks in
        self.task_keys order (finest first); entries at or beyond count are (-1, 0)."""
        logits = []
        for t, C_ in zip(self.task_keys, self.num_classes):
            x = outputs[t]
            if isinstance(x, dict):
                raise L.LnxError(f"DevicePredictor: dict-valued head output for {t} is not supported")
            if not x.is_cuda:
                raise L.LnxError(f"DevicePredictor: {t} logits are on {x.device}; linnaeus_amd has no CPU fallback")
            if x.dim() != 2 or x.shape[1] < C_:
                raise L.LnxError(f"DevicePredictor: {t} has logits of shape {tuple(x.shape)}, {C_} classes")
            logits.append(x.detach())
        first = logits[0]
        for i, x in enumerate(logits):  # mixed or other dtypes and strided columns: the only cases that cost a copy
            if x.dtype != first.dtype or x.dtype not in (torch.float32, torch.bfloat16):
                logits[i] = x = x.float() if first.dtype != torch.bfloat16 else x.to(torch.bfloat16)
            if x.shape[1] > 1 and x.stride(1) != 1:
                logits[i] = x.contiguous()
        K, kps = self._k_args(top_k, first.shape[0], first.device)
        parents, ids = self._tables_on(first.device)
        out = ops.predict_topk(logits, parents, K=K, null_index=self.null_index, id_maps=ids, k_per_sample=kps, consistency=self.consistency,
                               num_classes=self.num_classes)
        return dict(zip(("ids", "probs", "count", "flags"), out))

    def predict(self, model, images, aux=None, top_k=None) -> Dict[str, torch.Tensor]:
        """The model's eval / no_grad forward, then predict_logits on what it returns."""
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                outputs = model(images, aux)
        finally:
            model.train(was_training)
        return self.predict_logits(outputs, top_k)

    def to_results(self, pred) -> list:
        """ONE device-to-host copy of the four tensors -> per sample a list, coarsest task first (the reference's order), of
        (task_key, [(id, probability), ...]) with `count` entries each.  Plain Python types."""
        ids, probs, count = pred["ids"], pred["probs"], pred["count"]
        B, T, K = ids.shape
        # one copy: ids, then the probabilities' bit patterns, the counts and the flags, as int64
        both = torch.cat([ids.reshape(-1), probs.reshape(-1).view(torch.int32).to(torch.int64), count.reshape(-1).to(torch.int64),
                          pred["flags"].reshape(-1).to(torch.int64)]).cpu()
        n = B * T * K
        ids_h = both[:n].view(B, T, K).tolist()
        probs_h = both[n: 2 * n].to(torch.int32).view(torch.float32).view(B, T, K).tolist()
        count_h = both[2 * n: 2 * n + B * T].view(B, T).tolist()
        return [[(self.task_keys[t], list(zip(ids_h[b][t][: count_h[b][t]], probs_h[b][t][: count_h[b][t]]))) for t in range(T - 1, -1, -1)]
                for b in range(B)]
