"""Inference on the device.  DevicePreprocessor: a batch of images of any sizes -> the normalized fp32 input tensor in at most two HIP
launches, bit-identical to the reference's PIL / torchvision recipe (inference/preprocessing.py:29-82).  DevicePredictor, below:

Predictions on the device: one HIP launch per batch from {task: logits} to the final top-k lists, no host synchronisation.

DevicePredictor does what the reference's LinnaeusInferenceHandler.predict does after the forward (inference/handler.py:186-228: per
sample and task softmax, topk and two .item() per kept entry) and then enforce_hierarchical_consistency
(inference/postprocessing.py:14-171, a Python walk of the taxonomy tree per sample) with lnx_predict, which reads every logit once and
writes four device tensors.  to_results() copies them to the host once and returns plain Python lists.

What differs from the reference: probabilities are an fp32 softmax whatever the logits' dtype (the reference runs softmax in the
autocast dtype); equal values are ordered by ascending class index, NaN first; results are tuples, not `typus` objects; image and
metadata preprocessing and artifact loading are the caller's.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from . import ops
from .heads import parent_index_from_matrix


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
                    tab = parent_index_from_matrix(m)
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

    def predict_variants(self, model, images, metas, top_k=None) -> List[Dict[str, torch.Tensor]]:
        """`[predict(model, images, m, top_k) for m in metas]` for the price of one trunk pass: the model's eval / no_grad
        `forward_meta_variants` (the image alone against the image with its metadata, say), then one predict_logits per variant."""
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                outputs = model.forward_meta_variants(images, metas)
        finally:
            model.train(was_training)
        return [self.predict_logits(o, top_k) for o in outputs]

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


class DevicePreprocessor:
    """What the reference's preprocess_image_batch does (inference/preprocessing.py:29-82: per image TF.resize of a PIL image,
    TF.to_tensor, TF.normalize, then torch.stack and a pageable copy) with lnx_preprocess: the whole batch travels to the device in ONE
    copy from pinned memory and becomes fp32 [N, 3, H, W] there in at most two launches, in Pillow's own fixed-point arithmetic, so the
    result is the reference's bit for bit.  Nothing synchronises the device.

    What differs from the reference: an unknown interpolation name is refused (the reference silently takes bilinear), and so is an
    image with other than three channels; images may also be uint8 [h, w, 3] numpy arrays or CPU tensors; metadata preprocessing
    (preprocess_metadata_batch) stays the caller's."""

    FILTERS = {"nearest": L.RESIZE_NEAREST, "nearest_exact": L.RESIZE_NEAREST, "bilinear": L.RESIZE_BILINEAR, "bicubic": L.RESIZE_BICUBIC}
    _ALIGN = 16

    def __init__(self, image_size=(3, 224, 224), mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), interpolation: str = "bilinear", device=None):
        """image_size: (3, H, W) as INPUT.image_size of the reference's inference config; mean / std: per channel; interpolation:
        bilinear, bicubic, nearest or nearest_exact (the same as nearest for PIL inputs); device: default the current one."""
        size = [int(v) for v in image_size]
        if len(size) != 3 or size[0] != 3 or not all(1 <= v <= L.PREPROCESS_MAX_SIDE for v in size[1:]):
            raise L.LnxError(f"DevicePreprocessor: image_size={tuple(image_size)}; expected (3, H, W) with sides in 1..{L.PREPROCESS_MAX_SIDE}")
        name = str(interpolation).lower()
        if name not in self.FILTERS:
            raise L.LnxError(f"DevicePreprocessor: unknown interpolation {interpolation!r} (one of {sorted(self.FILTERS)})")
        self.H, self.W = size[1], size[2]
        self.interpolation, self.filter = name, self.FILTERS[name]
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        if len(self.mean) != 3 or len(self.std) != 3 or any(C.c_float(v).value == 0.0 for v in self.std):
            raise L.LnxError(f"DevicePreprocessor: mean={mean} std={std}; three values each, no zero std")
        self.device = device
        self._tables: Dict[tuple, np.ndarray] = {}  # (in, out) -> the axis tables as one int32 array (k rows, then bounds)
        self._pinned = [None, None]                 # two staging buffers used in turn, each with the event of its last copy
        self._copied = [None, None]
        self._turn = 0
        self._blob = self._scratch = self._done = None
        self.scratch_bytes = 0  # what the last call needed

    @classmethod
    def from_input_config(cls, input_cfg, device=None):
        """input_cfg: the reference's InputConfig or a mapping with image_size, image_mean, image_std, image_interpolation."""
        get = input_cfg.get if isinstance(input_cfg, dict) else lambda k: getattr(input_cfg, k)
        return cls(get("image_size"), get("image_mean"), get("image_std"), get("image_interpolation"), device=device)

    # ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _as_array(img, i: int) -> np.ndarray:
        if isinstance(img, (bytes, bytearray, memoryview)):  # _decode_image (preprocessing.py:19-26)
            from io import BytesIO

            from PIL import Image

            try:
                img = Image.open(BytesIO(img)).convert("RGB")
            except Exception as e:
                raise ValueError("Invalid image data") from e
        if isinstance(img, torch.Tensor):
            if img.is_cuda:
                raise L.LnxError(f"DevicePreprocessor: image {i} is a device tensor; sources are host uint8 [h, w, 3]")
            arr = img.detach().numpy()
        elif isinstance(img, np.ndarray):
            arr = img
        elif hasattr(img, "convert") and hasattr(img, "mode"):  # a PIL image (preprocessing.py:71)
            arr = np.asarray(img if img.mode == "RGB" else img.convert("RGB"))
        else:
            raise TypeError(f"Unsupported image type: {type(img)}. Expected bytes, a PIL image, a uint8 numpy array or a CPU tensor.")
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise L.LnxError(f"DevicePreprocessor: image {i} has shape {tuple(arr.shape)}; expected [h, w, 3] (three channels)")
        if arr.dtype != np.uint8:
            raise L.LnxError(f"DevicePreprocessor: image {i} is {arr.dtype}; expected uint8")
        if not all(1 <= v <= L.PREPROCESS_MAX_SIDE for v in arr.shape[:2]):
            raise L.LnxError(f"DevicePreprocessor: image {i} is {arr.shape[0]}x{arr.shape[1]}; sides must be in 1..{L.PREPROCESS_MAX_SIDE}")
        return arr

    def _axis_tables(self, in_size: int, out_size: int) -> np.ndarray:
        key = (in_size, out_size)
        tab = self._tables.get(key)
        if tab is None:
            lib = L.lib()
            if self.filter == L.RESIZE_NEAREST:
                tab = np.empty(out_size, np.int32)
                L.check(lib.lnx_resize_coeffs(in_size, out_size, self.filter, None, tab.ctypes.data), "lnx_resize_coeffs")
            else:
                taps = lib.lnx_resize_taps(in_size, out_size, self.filter)
                tab = np.empty(out_size * (taps + 2), np.int32)
                L.check(lib.lnx_resize_coeffs(in_size, out_size, self.filter, tab.ctypes.data, tab[out_size * taps:].ctypes.data), "lnx_resize_coeffs")
            if len(self._tables) >= 4096:
                self._tables.clear()
            self._tables[key] = tab
        return tab

    def _staging(self, nbytes: int):
        """The next of the two pinned buffers, at least nbytes long, once the copy that last read it has finished."""
        t = self._turn
        self._turn ^= 1
        if self._copied[t] is not None:
            self._copied[t].synchronize()  # the copy of two calls ago: long done unless the host runs far ahead of the device
        if self._pinned[t] is None or self._pinned[t].numel() < nbytes:
            self._pinned[t] = torch.empty(max(nbytes, 1 << 20) * 5 // 4, dtype=torch.uint8, pin_memory=True)
        return t, self._pinned[t]

    def __call__(self, images) -> torch.Tensor:
        """images: a list of uint8 [h, w, 3] numpy arrays / CPU tensors, PIL images or encoded bytes, of any sizes -> fp32
        [N, 3, H, W] on the device.  One host-to-device copy and at most two launches on the current stream; no synchronisation."""
        arrays = [self._as_array(img, i) for i, img in enumerate(images)]
        if not torch.cuda.is_available():
            raise L.LnxError("DevicePreprocessor needs a HIP device: linnaeus_amd has no CPU fallback")
        device = torch.device(self.device) if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        n, H, W, A = len(arrays), self.H, self.W, self._ALIGN
        if n == 0:  # preprocessing.py:78-80
            return torch.empty((0, 3, H, W), dtype=torch.float32, device=device)
        pad = lambda v: (v + A - 1) // A * A  # noqa: E731
        # layout of the blob: descriptors, the tables of every distinct axis, the sources
        nearest = self.filter == L.RESIZE_NEAREST
        off = pad(n * C.sizeof(L.PreprocessImage))
        table_at, tables = {}, []
        for arr in arrays:
            for in_size, out_size in ((arr.shape[1], W), (arr.shape[0], H)):
                if (in_size, out_size) not in table_at and (nearest or in_size != out_size):
                    tab = self._axis_tables(in_size, out_size)
                    table_at[(in_size, out_size)] = (off, 4 * (tab.size - 2 * out_size))  # where the table starts, bytes of k in front of bounds
                    tables.append((off, tab))
                    off = pad(off + tab.nbytes)
        src_at = []
        for arr in arrays:
            src_at.append(off)
            off = pad(off + arr.shape[0] * arr.shape[1] * 3)
        nbytes = off
        turn, pinned = self._staging(nbytes)
        host = pinned.numpy()
        descs = (L.PreprocessImage * n).from_buffer(host)
        for d, arr, at in zip(descs, arrays, src_at):
            h, w = arr.shape[:2]
            d.src, d.h, d.w = at, h, w
            d.hk = d.hb = d.vk = d.vb = 0
            if nearest or w != W:
                d.hk, k_bytes = table_at[(w, W)]
                d.hb = d.hk if nearest else d.hk + k_bytes
            if nearest or h != H:
                d.vk, k_bytes = table_at[(h, H)]
                d.vb = d.vk if nearest else d.vk + k_bytes
            np.copyto(host[at: at + h * w * 3].reshape(h, w, 3), arr)
        for at, tab in tables:
            host[at: at + tab.nbytes].view(np.int32)[:] = tab
        scratch_bytes = L.lib().lnx_preprocess_scratch_bytes(descs, n, H, W, self.filter)
        self.scratch_bytes = scratch_bytes
        if scratch_bytes < 0:
            raise L.LnxError(f"lnx_preprocess_scratch_bytes failed: {L.lib().lnx_last_error().decode()}")
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream()
            if self._done is not None:
                stream.wait_event(self._done)  # the device buffers are reused: behind the kernels of the call before, on any stream
            if self._blob is None or self._blob.numel() < nbytes or self._blob.device != device:
                self._blob = torch.empty(pinned.numel(), dtype=torch.uint8, device=device)
            if scratch_bytes and (self._scratch is None or self._scratch.numel() < scratch_bytes or self._scratch.device != device):
                self._scratch = torch.empty(scratch_bytes * 5 // 4, dtype=torch.uint8, device=device)
            self._blob[:nbytes].copy_(pinned[:nbytes], non_blocking=True)
            if self._copied[turn] is None:
                self._copied[turn] = torch.cuda.Event()
            self._copied[turn].record(stream)
            out = torch.empty((n, 3, H, W), dtype=torch.float32, device=device)
            ops.preprocess_images(self._blob, nbytes, descs, 0, n, H, W, self.filter, self.mean, self.std, self._scratch if scratch_bytes else None, out)
            if self._done is None:
                self._done = torch.cuda.Event()
            self._done.record(stream)
        del descs
        return out


def input_attribution(model, images, aux=None, task=None, class_index=None, kind: str = "grad"):
    """Which pixels and which metadata components a class logit depends on: one eval-mode forward and one backward of the HIP plan with
    the inputs as the differentiated leaves (the plan's backward then runs down to the image and to the metadata, whatever is frozen:
    `lnx_plan_set_input_grads`), seeded with the chosen logit of every sample.

    task: a key of the model's output dict (default: the first task); class_index: an int, a [B] integer tensor, or None = each
    sample's predicted (argmax) class of `task`.  kind = "grad": `image` is the channel-max of |d logit / d image|; "grad_x_input": the
    channel-sum of gradient * image.  Returns {"image": [B, H, W], "meta": {component: [B]}}; `meta` holds the L2 norm of each metadata
    component's slice of d logit / d aux (empty for a model without metadata components).  First-order only."""
    if kind not in ("grad", "grad_x_input"):
        raise ValueError(f"kind must be 'grad' or 'grad_x_input', got {kind!r}")
    has_meta = bool(getattr(model, "use_meta", False) and getattr(model, "meta_dims", None))
    x = images.detach().float().contiguous().requires_grad_(True)
    m = aux.detach().float().contiguous().requires_grad_(True) if (has_meta and aux is not None) else aux
    was_training = model.training
    model.eval()
    try:
        with torch.enable_grad():
            out = model(x, m)
            key = task if task is not None else next(iter(out))
            if key not in out:
                raise KeyError(f"unknown task {key!r}; the model's tasks are {list(out)}")
            logits = out[key].float()
            if class_index is None:
                idx = logits.detach().argmax(-1)
            elif isinstance(class_index, int):
                idx = torch.full((logits.shape[0],), class_index, device=logits.device, dtype=torch.long)
            else:
                idx = torch.as_tensor(class_index, device=logits.device).long().reshape(-1)
            seed = logits.gather(1, idx.unsqueeze(1)).sum()
            leaves = [x] + ([m] if (has_meta and m is not None) else [])
            grads = torch.autograd.grad(seed, leaves)
    finally:
        model.train(was_training)
    dx = grads[0]
    image = dx.abs().amax(1) if kind == "grad" else (dx * x.detach()).sum(1)
    meta = {}
    if len(grads) > 1:
        for name, info in model.meta_components.items():
            meta[name] = grads[1][:, info["offset"]: info["offset"] + info["dim"]].norm(dim=1)
    return {"image": image, "meta": meta}
