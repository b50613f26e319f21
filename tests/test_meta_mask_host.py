"""Metadata masking on device, the parts that need no GPU: the whitelist -> bitmask / threshold tables, how the probabilities are
read from a schedule, every refusal of the Python layer and of lnx_meta_mask, and the fixture's own consistency -- the numpy
restatement of the rule (tests/meta_mask_ref.py) reproduces what the reference returned from the draws it recorded, so a wrong
fixture cannot hide behind the kernel."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import collate as K
from tests import meta_mask_ref as R

BOUNDS = {"TEMPORAL": (0, 2), "SPATIAL": (2, 5), "ELEVATION": (5, 15)}
NAMES = list(BOUNDS)


# --- tables -------------------------------------------------------------------------------------------------------------------------


def test_tables_of_the_example_whitelist():
    wl = [["TEMPORAL"], ["SPATIAL"], ["ELEVATION"], ["TEMPORAL", "SPATIAL"], ["TEMPORAL", "ELEVATION"], ["SPATIAL", "ELEVATION"]]
    bits, thr = K.partial_mask_tables(NAMES, wl, [1.0, 1.0, 1.0, 0.5, 0.5, 0.5])
    assert bits == [1, 2, 4, 3, 5, 6]
    want = np.cumsum([1.0, 1.0, 1.0, 0.5, 0.5, 0.5]) / 4.5
    assert thr == [float(np.float32(v)) for v in want[:-1]] + [1.0]
    assert all(a < b for a, b in zip(thr, thr[1:])) and thr[-1] == 1.0


def test_weights_of_another_length_give_a_uniform_pick():
    wl = [["TEMPORAL"], ["SPATIAL"], ["ELEVATION"]]
    for weights in (None, [], [1.0, 5.0], [1.0, 2.0, 3.0, 4.0]):
        bits, thr = K.partial_mask_tables(NAMES, wl, weights)
        assert bits == [1, 2, 4] and thr == [float(np.float32(1 / 3)), float(np.float32(2 / 3)), 1.0], weights


def test_last_threshold_is_forced_to_one_and_zero_weights_are_never_picked():
    bits, thr = K.partial_mask_tables(NAMES, [["TEMPORAL"], ["SPATIAL"], ["ELEVATION"]], [0.0, 0.1, 0.2])
    assert thr[0] == 0.0 and thr[-1] == 1.0  # no draw is < 0: the first combination is never picked
    u = np.array([0.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    assert R.pick_ref(thr, u).tolist() == [1, 2]


def test_empty_whitelist_and_unknown_names():
    assert K.partial_mask_tables(NAMES, [], [1.0]) == ([], [])
    assert K.partial_mask_tables(NAMES, None, None) == ([], [])
    bits, thr = K.partial_mask_tables(NAMES, [["TEMPORAL", "WEATHER"], ["WEATHER"], ["SPATIAL", "SPATIAL"]], [1.0, 2.0, 1.0])
    assert bits == [1, 0, 2]  # unknown names are dropped, the combination keeps its place and its weight
    assert thr == [0.25, 0.75, 1.0]


def test_tables_are_read_from_the_schedule_when_not_given():
    sched = SimpleNamespace(meta_cfg=SimpleNamespace(PARTIAL=SimpleNamespace(WHITELIST=[["SPATIAL"], ["ELEVATION"]], WEIGHTS=[3.0, 1.0])))
    m = K.GPUMetaMasking(BOUNDS, sched)
    assert m.combo_bits == [2, 4] and m.combo_thr == [0.75, 1.0]
    m = K.GPUMetaMasking(BOUNDS, sched, whitelist=[["TEMPORAL"]], weights=[2.0])
    assert m.combo_bits == [1] and m.combo_thr == [1.0]
    m = K.GPUMetaMasking(BOUNDS, SimpleNamespace(meta_cfg={"PARTIAL": {"WHITELIST": [["TEMPORAL"]]}}))  # mappings work as well
    assert m.combo_bits == [1]
    assert K.GPUMetaMasking(BOUNDS).combo_bits == []
    assert m.components == NAMES and m.bounds == [(0, 2), (2, 5), (5, 15)]


# --- schedule -----------------------------------------------------------------------------------------------------------------------


class _Sched:
    def __init__(self, step=7):
        self.training_progress = SimpleNamespace(global_step=step)
        self.asked = []

    def get_meta_mask_prob(self, step):
        self.asked.append(("plain", step))
        return 0.25

    def get_partial_mask_enabled(self):
        return True

    def get_partial_meta_mask_prob(self):
        return 0.5


class _SchedByIteration(_Sched):
    def get_meta_mask_prob_by_iteration(self, step):
        self.asked.append(("by_iteration", step))
        return 0.75


def test_probabilities_come_from_the_schedule():
    s = _Sched()
    assert K.GPUMetaMasking(BOUNDS, s).probabilities() == (0.25, True, 0.5)
    assert s.asked == [("plain", 7)]  # step defaults to training_progress.global_step
    assert K.GPUMetaMasking(BOUNDS, s).probabilities(3) == (0.25, True, 0.5) and s.asked[-1] == ("plain", 3)


def test_by_iteration_getter_is_preferred():
    s = _SchedByIteration()
    assert K.GPUMetaMasking(BOUNDS, s).probabilities(11) == (0.75, True, 0.5)
    assert s.asked == [("by_iteration", 11)]


def test_partial_probability_defaults_to_one():
    s = SimpleNamespace(get_meta_mask_prob=lambda step: 0.0, get_partial_mask_enabled=lambda: False)
    assert K.GPUMetaMasking(BOUNDS, s).probabilities(0) == (0.0, False, 1.0)  # no training_progress: step given
    assert K.GPUMetaMasking(BOUNDS, s).probabilities() == (0.0, False, 1.0)  # ... or 0
    with pytest.raises(ValueError, match="ops_schedule"):
        K.GPUMetaMasking(BOUNDS).probabilities()


# --- refusals of the Python layer ---------------------------------------------------------------------------------------------------


def test_python_layer_refusals():
    with pytest.raises(ValueError, match="at most 32"):
        K.GPUMetaMasking({f"c{i}": (i, i + 1) for i in range(33)})
    K.GPUMetaMasking({f"c{i}": (i, i + 1) for i in range(32)})
    with pytest.raises(ValueError, match="non-negative"):
        K.GPUMetaMasking(BOUNDS, whitelist=[["TEMPORAL"], ["SPATIAL"]], weights=[1.0, -0.5])
    with pytest.raises(ValueError, match="sum to 0"):
        K.GPUMetaMasking(BOUNDS, whitelist=[["TEMPORAL"], ["SPATIAL"]], weights=[0.0, 0.0])
    K.GPUMetaMasking(BOUNDS, whitelist=[["TEMPORAL"], ["SPATIAL"]], weights=[-1.0])  # another length: the weights are not used at all
    m = K.GPUMetaMasking(BOUNDS)
    m._shape(torch.zeros(2, 15))
    m._shape(torch.zeros(2, 17))
    with pytest.raises(ValueError, match=r"outside \[0, 14\]"):
        m._shape(torch.zeros(2, 14))
    with pytest.raises(ValueError, match="outside"):
        K.GPUMetaMasking({"a": (3, 2)})._shape(torch.zeros(2, 15))
    with pytest.raises(ValueError, match="outside"):
        K.GPUMetaMasking({"a": (-1, 2)})._shape(torch.zeros(2, 15))


def test_there_is_no_cpu_path():
    aux, masks = torch.randn(4, 15), torch.ones(4, 15, dtype=torch.bool)
    with pytest.raises(L.LnxError, match="HIP kernels only"):
        K.GPUMetaMasking(BOUNDS)(aux, masks, p_full=0.5, partial_enabled=False, p_partial=0.0)
    with pytest.raises(L.LnxError, match="HIP kernels only"):
        K.GPUMetaMasking(BOUNDS).stats(masks)
    with pytest.raises(L.LnxError, match="HIP kernels only"):
        K.mask_meta_components(aux, BOUNDS)


def test_exported_from_the_package():
    import linnaeus_amd

    assert linnaeus_amd.GPUMetaMasking is K.GPUMetaMasking and linnaeus_amd.GPUTrainCollate is K.GPUTrainCollate
    assert linnaeus_amd.mask_meta_components is K.mask_meta_components


# --- lnx_meta_mask argument validation (host side of the entry point: no pointer below is dereferenced) -----------------------------


def _args(**kw):
    fake = 0x1000
    a = L.MetaMaskArgs()
    a.aux = a.mask = a.out_aux = a.out_mask = a.bounds = a.draws = a.combo_bits = a.combo_thr = fake
    a.B, a.D, a.ncomp, a.ncombo = 8, 15, 3, 6
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("change, message", [
    (dict(B=0), b"bad shape"), (dict(B=-3), b"bad shape"), (dict(D=0), b"bad shape"),
    (dict(ncomp=33), b"33 components"), (dict(ncomp=-1), b"components"),
    (dict(bounds=None), b"null component bounds"),
    (dict(aux=None), b"null aux"), (dict(mask=None), b"null mask"), (dict(mask=None, out_mask=None, counts=0x1000), b"null mask"),
    (dict(out_aux=None, out_mask=None), b"null outputs"),
    (dict(combo_bits=None), b"null combination table"), (dict(combo_thr=None), b"null combination table"), (dict(ncombo=-1), b"combination table"),
    (dict(row_bits=1), b"without draws"), (dict(row_full=1), b"without draws"),
    (dict(draws=None, combo_idx=0x1000), b"combo_idx needs draws"),
    (dict(draws=None, p_full=0.5), b"null draws"), (dict(draws=None, partial_on=1), b"null draws"),
])
def test_entry_point_refuses(change, message):
    lib = L.lib()
    assert lib.lnx_meta_mask(C.byref(_args(**change)), None) != 0, change
    assert message in lib.lnx_last_error(), (change, lib.lnx_last_error())


def test_entry_point_refuses_a_null_struct_and_knows_its_version():
    lib = L.lib()
    assert lib.lnx_meta_mask(None, None) != 0 and b"null argument" in lib.lnx_last_error()
    assert lib.lnx_version() >= 108
    assert L.META_MASK_MAX_COMPONENTS == 32


def test_ctypes_mirror_has_the_size_the_c_compiler_gives(tmp_path):
    import os
    import shutil
    import subprocess

    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "lnx.h"\nint main(void) { printf("%zu %d\\n", sizeof(lnx_meta_mask_args), LNX_META_MASK_MAX_COMPONENTS); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-I", os.path.join(os.path.dirname(R.GOLDEN), "..", "..", "include"), str(src), "-o", str(exe)], check=True)
    size, ncomp = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == C.sizeof(L.MetaMaskArgs) and int(ncomp) == L.META_MASK_MAX_COMPONENTS


# --- the fixture ----------------------------------------------------------------------------------------------------------------------


def test_fixture_holds_the_cases_the_masking_is_specified_on():
    names = R.case_names()
    assert names == ["mixed", "one", "all_full", "no_full", "partial_off", "unknown_name", "empty_whitelist", "uniform_pick", "dirty_inputs", "uncovered"]
    c = R.case("mixed")
    assert c["aux"].shape == (8, 15) and int((c["draws"][0] < 0.3).sum()) == 2 and int((c["combo_idx"] >= 0).sum()) == 6
    assert R.case("one")["aux"].shape == (1, 15) and R.case("uncovered")["aux"].shape == (8, 17)
    assert bool(R.case("all_full")["out_masks"].any()) is False and not R.case("all_full")["out_aux"].any()
    assert (R.case("no_full")["combo_idx"] >= 0).any() and (R.case("partial_off")["combo_idx"] == -1).all()
    assert R.case("unknown_name")["combo_bits"].tolist() == [1, 0, 2] and len(R.case("empty_whitelist")["combo_bits"]) == 0
    d = R.case("dirty_inputs")
    assert not d["masks"].all() and (d["aux"] == 0).any()
    u = R.case("uncovered")
    assert (u["out_aux"][:, 15:] != 0).any() and not u["out_aux"][u["draws"][0] < 0.3, 15:].any()  # cleared by a full mask only


@pytest.mark.parametrize("name", R.case_names())
def test_numpy_restatement_reproduces_the_reference(name):
    c = R.case(name)
    p_full, partial, p_partial = c["p"]
    out_aux, out_masks, counts, k = R.meta_mask_ref(c["aux"], c["masks"], c["bounds"], c["combo_bits"], c["draws"], p_full, partial, p_partial, combo_idx=c["combo_idx"])
    assert out_aux.tobytes() == c["out_aux"].tobytes()
    assert np.array_equal(out_masks, c["out_masks"]) and out_masks.dtype == np.bool_
    assert R.stats_ref(out_masks, c["bounds"]).tobytes() == c["stats"].tobytes()
    assert np.array_equal(k, c["combo_idx"])  # the recorded picks sit exactly on the rows the draws make partial
    assert counts[0] == int((c["draws"][0] < np.float32(p_full)).sum())


@pytest.mark.parametrize("k", [0, 1])
def test_numpy_restatement_reproduces_the_evaluation_slicing(k):
    z = R.golden()
    aux, bounds = z[f"eval{k}_aux"], z[f"eval{k}_bounds"]
    out = aux.copy()
    if int(z[f"eval{k}_all"]):
        out[:] = 0
    else:
        out[:, (R.column_bits(bounds, aux.shape[1]) & np.uint64(int(z[f"eval{k}_bits"]))) != 0] = 0
    assert out.tobytes() == z[f"eval{k}_out"].tobytes()
    assert int(z["eval0_bits"]) == 6 and int(z["eval1_all"]) == 1
