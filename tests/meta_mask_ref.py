"""All-numpy restatement of the metadata-masking rule (include/lnx.h, lnx_meta_mask) and access to tests/golden/meta_mask.npz,
shared by tests/test_meta_mask_host.py (which checks the restatement against the reference's recorded outputs) and
tests/test_gpu_meta_mask.py (which checks the kernel against both).  Nothing here imports linnaeus_amd."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meta_mask.npz")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def case_names():
    return [str(n) for n in golden()["cases"]]


def case(name):
    z = golden()
    return {k[len(name) + 1:]: v for k, v in z.items() if k.startswith(name + "_")}


def bounds_map(c):
    return {str(n): (int(s), int(e)) for n, (s, e) in zip(c["components"], c["bounds"])}


def whitelist_of(c):
    """the recorded bitmasks as lists of component names (unknown names are already dropped in the fixture)"""
    names = [str(n) for n in c["components"]]
    return [[n for i, n in enumerate(names) if (int(b) >> i) & 1] for b in c["combo_bits"]]


def pick_ref(thr, u):
    """first k with u < thr[k], the last entry when there is none: numpy.searchsorted on the same fp32 thresholds"""
    thr = np.asarray(thr, np.float32)
    return np.minimum(np.searchsorted(thr, np.asarray(u, np.float32), side="right"), len(thr) - 1).astype(np.int32)


def column_bits(bounds, D):
    cb = np.zeros(D, np.uint64)
    for c, (s, e) in enumerate(bounds):
        cb[int(s):int(e)] |= np.uint64(1 << c)
    return cb


def counts_ref(out_masks, bounds):
    out_masks = np.asarray(out_masks) != 0
    return np.array([int(out_masks[:, int(s):int(e)].all(axis=1).sum()) for s, e in bounds], np.int32)


def meta_mask_ref(aux, masks, bounds, combo_bits, draws, p_full, partial_on, p_partial, combo_idx=None, thr=None):
    """-> (out_aux, out_masks, counts int32[2 + ncomp], row_combo int32[B]); comparisons in fp32 and strict, as the kernel's"""
    aux, masks = np.asarray(aux), np.asarray(masks)
    B, D = aux.shape
    draws = np.asarray(draws, np.float32)
    full = draws[0] < np.float32(p_full)
    partial = ~full & bool(partial_on) & (draws[1] < np.float32(p_partial))
    ncombo = len(combo_bits)
    if combo_idx is not None:
        k = np.asarray(combo_idx, np.int32).copy()
    elif ncombo:
        k = pick_ref(thr, draws[2])
    else:
        k = np.full(B, -1, np.int32)
    k[~partial] = -1
    k[(k < 0) | (k >= ncombo)] = -1
    row_bits = np.array([int(combo_bits[i]) if i >= 0 else 0 for i in k], np.uint64)
    clear = full[:, None] | ((row_bits[:, None] & column_bits(bounds, D)[None, :]) != 0)
    out_aux = np.where(clear, np.float32(0), aux).astype(aux.dtype)
    out_masks = np.where(clear, np.zeros((), masks.dtype), masks)
    counts = np.concatenate([np.array([full.sum(), (k >= 0).sum()], np.int32), counts_ref(out_masks, bounds)]).astype(np.int32)
    return out_aux, out_masks, counts, k


def stats_ref(out_masks, bounds):
    """actual_meta_stats of the reference: (valid_count / B) * 100.0 in double"""
    return np.array([(int(n) / out_masks.shape[0]) * 100.0 for n in counts_ref(out_masks, bounds)], np.float64)
