#!/usr/bin/env python3
"""Generate tests/golden/meta_mask.npz from the reference's own collate step (linnaeus/h5data/h5dataloader.py
H5DataLoader.collate_fn: full masking :709-797, partial masking :798-940 with _apply_partial_mask :366-482, component statistics
:1677-1801; the pick is OpsSchedule.pick_partial_mask_combo, linnaeus/ops_schedule/ops_schedule.py:628-650) and from the slicing of
linnaeus/validation.py (:174-175 mask_meta, :428-489 validate_with_partial_mask).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_meta_mask.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/ and two empty module stand-ins made here
(h5py, cv2: imported by the dataset modules, never called) and runs on CPU.  Run by hand, never by a test.

collate_fn is driven without H5DataLoader's constructor (which wants a prefetching dataset and a sampler): an instance from
object.__new__ gets exactly the attributes the method reads.  The schedule is a stand-in with the four getters collate_fn calls and
`get_mixup_prob -> 0` (no mixing; it has no `config`, so the sampler-type branch is the legacy one); its pick_partial_mask_combo IS
the reference's method, called on the stand-in (it reads meta_cfg.PARTIAL only), wrapped to record each pick.

The uniform draws are recovered by re-seeding: collate_fn draws `torch.rand(B)` for the full mask only when p_full > 0, then
`torch.rand(B)` for the partial mask only when partial masking is on with p_partial > 0.  A draw the reference did not make is
recorded as 0.5 (it decides nothing: the matching probability is 0 or the stage is off).  The third row of `draws` (the
combination draw of the device path) is not something the reference has: it is 0, and `combo_idx` replays the recorded picks.

Per case NAME the file holds arrays only:
  NAME_aux [B, D] f32, NAME_masks [B, D] bool        inputs
  NAME_bounds [ncomp, 2] i32, NAME_components [ncomp] component names in map order
  NAME_combo_bits [ncombo] u32                        whitelist as bitmasks over the components (unknown names dropped)
  NAME_weights [ncombo or 0] f64                      WEIGHTS as configured
  NAME_p [3] f64                                      p_full, partial_enabled, p_partial
  NAME_draws [3, B] f32, NAME_combo_idx [B] i32       u_full, u_partial, 0; whitelist index picked per row, -1 where none
  NAME_out_aux, NAME_out_masks                        what collate_fn returned
  NAME_stats [ncomp] f64                              actual_meta_stats in map order
and for the two evaluation cases evalK_aux, evalK_bounds, evalK_components, evalK_bits (u32; evalK_all = 1: everything), evalK_out.
The archive is written with fixed zip timestamps, so the same inputs give the same bytes.
"""
import io
import os
import random
import sys
import types
import zipfile
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "h5data", "h5dataloader.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(HERE, "_stubs"), REF]
sys.dont_write_bytecode = True
for name in ("h5py", "cv2"):
    sys.modules.setdefault(name, types.ModuleType(name))

import contextlib  # noqa: E402
import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

warnings.filterwarnings("ignore")
logging.disable(logging.CRITICAL)

from linnaeus.h5data.h5dataloader import H5DataLoader  # noqa: E402
from linnaeus.ops_schedule.ops_schedule import OpsSchedule  # noqa: E402
from linnaeus.validation import get_component_bounds  # noqa: E402

BOUNDS15 = {"TEMPORAL": (0, 2), "SPATIAL": (2, 5), "ELEVATION": (5, 15)}
WHITELIST6 = [["TEMPORAL"], ["SPATIAL"], ["ELEVATION"], ["TEMPORAL", "SPATIAL"], ["TEMPORAL", "ELEVATION"], ["SPATIAL", "ELEVATION"]]
WEIGHTS6 = [1.0, 1.0, 1.0, 0.5, 0.5, 0.5]

# name: B, D, p_full, partial_enabled, p_partial, whitelist, weights, input seed, dirty inputs
CASES = {
    "mixed": dict(B=8, p_full=0.3, partial=True, p_partial=0.7),
    "one": dict(B=1, p_full=0.3, partial=True, p_partial=0.7, seed=3),
    "all_full": dict(B=8, p_full=1.0, partial=True, p_partial=0.7),
    "no_full": dict(B=8, p_full=0.0, partial=True, p_partial=0.7),
    "partial_off": dict(B=8, p_full=0.3, partial=False, p_partial=0.7),
    "unknown_name": dict(B=8, p_full=0.3, partial=True, p_partial=0.7, whitelist=[["TEMPORAL", "WEATHER"], ["WEATHER"], ["SPATIAL"]], weights=[1.0, 2.0, 1.0]),
    "empty_whitelist": dict(B=8, p_full=0.3, partial=True, p_partial=0.7, whitelist=[], weights=[]),
    "uniform_pick": dict(B=8, p_full=0.1, partial=True, p_partial=1.0, weights=[1.0, 2.0]),  # length mismatch: random.choice
    "dirty_inputs": dict(B=8, p_full=0.3, partial=True, p_partial=0.7, dirty=True),
    "uncovered": dict(B=8, D=17, p_full=0.3, partial=True, p_partial=0.7),
}


class Schedule:
    """what collate_fn asks of an OpsSchedule, and nothing else"""

    def __init__(self, p_full, partial, p_partial, whitelist, weights):
        self.p = (p_full, partial, p_partial)
        self.meta_cfg = SimpleNamespace(PARTIAL=SimpleNamespace(WHITELIST=whitelist, WEIGHTS=weights))
        self.training_progress = SimpleNamespace(global_step=0)
        self.picks = []

    def get_meta_mask_prob(self, step):
        return self.p[0]

    def get_partial_mask_enabled(self):
        return self.p[1]

    def get_partial_meta_mask_prob(self):
        return self.p[2]

    def get_mixup_prob(self, step):
        return 0.0

    def pick_partial_mask_combo(self):
        combo = OpsSchedule.pick_partial_mask_combo(self)  # the reference's method on this object
        self.picks.append(combo)
        return combo


def bare_loader(schedule, bounds_map):
    dl = object.__new__(H5DataLoader)
    dl.is_training = True
    dl.ops_schedule = schedule
    dl.config = None
    dl.batch_idx = 10  # past the first-batches diagnostics
    dl.current_epoch = 0
    dl.meta_chunk_bounds_map = dict(bounds_map)
    dl.meta_chunk_bounds_list = [list(v) for v in bounds_map.values()]
    dl.use_gpu = False
    dl.main_logger = logging.getLogger("meta_mask.main")
    dl.h5data_logger = logging.getLogger("meta_mask.h5data")
    return dl


def make_inputs(B, D, seed, dirty):
    g = torch.Generator().manual_seed(1000 + seed)
    aux = torch.randn(B, D, generator=g)
    aux[aux == 0] = 1.0
    masks = torch.ones(B, D, dtype=torch.bool)
    if dirty:  # components already invalid (zeros and False over a whole component), single False entries, zeros under a True mask
        drop = torch.rand(B, D, generator=g) < 0.2
        masks[drop] = False
        aux[drop] = 0.0
        masks[1, 2:5] = False
        aux[1, 2:5] = 0.0
        aux[2, 7] = 0.0
        masks[3, 0] = False
    return aux, masks


def run_case(name, B, p_full, partial, p_partial, D=15, whitelist=None, weights=None, seed=0, dirty=False):
    whitelist = WHITELIST6 if whitelist is None else whitelist
    weights = WEIGHTS6 if weights is None else weights
    bounds_map = BOUNDS15
    comps = list(bounds_map)
    aux, masks = make_inputs(B, D, seed, dirty)
    sched = Schedule(p_full, partial, p_partial, whitelist, weights)
    dl = bare_loader(sched, bounds_map)
    samples = [(torch.zeros(1, 2, 2), {"taxa_L10": torch.tensor([0.0, 1.0])}, aux[i].clone(), i, {}, masks[i].clone()) for i in range(B)]
    torch.manual_seed(seed)
    random.seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        out = dl.collate_fn(samples)
    out_aux, out_masks, stats = out[2], out[5], out[6]
    # the draws collate_fn made, in its order
    torch.manual_seed(seed)
    u_full = torch.rand(B) if p_full > 0 else torch.full((B,), 0.5)
    u_partial = torch.rand(B) if (partial and p_partial > 0) else torch.full((B,), 0.5)
    full = u_full < p_full
    eligible = [i for i in range(B) if partial and p_partial > 0 and not bool(full[i]) and bool(u_partial[i] < p_partial)]
    assert len(eligible) == len(sched.picks), (name, eligible, sched.picks)
    combo_idx = np.full(B, -1, np.int32)
    for i, combo in zip(eligible, sched.picks):
        combo_idx[i] = whitelist.index(combo) if combo else -1
    bits = np.array([sum(1 << comps.index(c) for c in set(combo) if c in comps) for combo in whitelist], np.uint32)
    n_partial = int((combo_idx >= 0).sum())
    print(f"[meta_mask/{name}] B {B} D {D}: {int(full.sum())} full, {n_partial} partial, picks {combo_idx.tolist()}, stats {stats}")
    return {
        f"{name}_aux": aux.numpy(), f"{name}_masks": masks.numpy(),
        f"{name}_bounds": np.array(list(bounds_map.values()), np.int32), f"{name}_components": np.array(comps),
        f"{name}_combo_bits": bits, f"{name}_weights": np.array(weights, np.float64),
        f"{name}_p": np.array([p_full, float(partial), p_partial], np.float64),
        f"{name}_draws": torch.stack([u_full, u_partial, torch.zeros(B)]).numpy(), f"{name}_combo_idx": combo_idx,
        f"{name}_out_aux": out_aux.numpy(), f"{name}_out_masks": out_masks.numpy(),
        f"{name}_stats": np.array([stats[c] for c in comps], np.float64),
    }


def eval_cases():
    """validation.py: mask_meta zeroes aux_info (:174-175); validate_with_partial_mask zeroes [start, end) of every listed component
    (:428-433 bounds from get_component_bounds over DATA.META.COMPONENTS, :472-473 the assignment)"""
    comps_cfg = SimpleNamespace(**{n: SimpleNamespace(IDX=s, DIM=e - s) for n, (s, e) in BOUNDS15.items()})
    comps = list(BOUNDS15)
    aux, _ = make_inputs(8, 15, 7, False)
    rec = {}
    for k, listed in enumerate((["ELEVATION", "SPATIAL"], None)):
        if listed is None:
            out = torch.zeros_like(aux)
        else:
            out = aux.clone()
            for start_idx, end_idx in [get_component_bounds(comps_cfg, c) for c in listed]:
                out[:, start_idx:end_idx] = 0.0
        rec.update({f"eval{k}_aux": aux.numpy(), f"eval{k}_bounds": np.array(list(BOUNDS15.values()), np.int32), f"eval{k}_components": np.array(comps),
                    f"eval{k}_bits": np.array(sum(1 << comps.index(c) for c in (listed or [])), np.uint32), f"eval{k}_all": np.array(int(listed is None), np.int32),
                    f"eval{k}_out": out.numpy()})
    return rec


def write_npz(path, rec):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same file"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(rec):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(rec[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    rec = {"cases": np.array(list(CASES))}
    for name, kw in CASES.items():
        rec.update(run_case(name, **kw))
    rec.update(eval_cases())
    out = os.path.join(REPO, "tests", "golden", "meta_mask.npz")
    write_npz(out, rec)
    print(f"wrote {out} ({os.path.getsize(out)} bytes, {len(rec)} arrays)")


if __name__ == "__main__":
    main()
