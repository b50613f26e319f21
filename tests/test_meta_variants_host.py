"""Metadata variants from one trunk pass, the parts that need no GPU: the refusals of lnx_plan_forward_tail (made before any launch,
no pointer is dereferenced), the trunk flag of a fresh plan, and the variant / phase-name helpers of linnaeus_amd.collate."""
import ctypes as C

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import collate

BOUNDS = {"TEMPORAL": (0, 2), "SPATIAL": (2, 5), "ELEVATION": (5, 15)}
ONE = C.c_void_p(16)  # a non-NULL pointer that must never be dereferenced


def make_plan(inference=1, n_meta=2, n_tasks=1, recompute=0):
    from linnaeus_amd.model import _Cfg

    cfg = _Cfg()
    cfg.dtype, cfg.batch, cfg.img_h, cfg.img_w, cfg.in_chans = L.BF16, 2, 64, 64, 3
    cfg.dims[:] = [32, 64, 128, 256]
    cfg.conv_depths[:] = [1, 1]
    cfg.rope_depths[:] = [2, 1]
    cfg.rope_heads[:] = [2, 4]
    cfg.mlp_hidden[:] = [512, 1024]
    cfg.n_meta = n_meta
    for i, d in enumerate((2, 3)[:n_meta]):
        cfg.meta_dims[i] = d
    cfg.n_tasks = n_tasks
    for i in range(n_tasks):
        cfg.task_classes[i] = 7
    cfg.inference, cfg.recompute = inference, recompute
    h = C.c_void_p()
    assert L.lib().lnx_plan_create(C.byref(cfg), C.byref(h)) == 0, L.lib().lnx_last_error()
    return h


def tail(h, meta=ONE, feats=ONE, logits=ONE):
    rc = L.lib().lnx_plan_forward_tail(h, meta, feats, logits, None)
    return rc, L.lib().lnx_last_error().decode()


def test_the_entry_points_are_exported():
    lib = L.lib()
    assert lib.lnx_version() >= 120
    assert "lnx_plan_forward_tail" in L.EXPORTS and "lnx_plan_trunk_valid" in L.EXPORTS


def test_a_null_plan_is_refused():
    rc, err = tail(None)
    assert rc != 0 and "bound" in err
    assert L.lib().lnx_plan_trunk_valid(None) == 0


def test_a_fresh_plan_has_no_trunk_and_an_unbound_plan_is_refused_by_name():
    lib = L.lib()
    h = make_plan()
    try:
        assert lib.lnx_plan_trunk_valid(h) == 0
        rc, err = tail(h)  # every argument in order: what is missing is the binding, and with it the trunk
        assert rc != 0 and "bound" in err and "trunk" in err
        assert lib.lnx_plan_trunk_valid(h) == 0
    finally:
        lib.lnx_plan_destroy(h)


@pytest.mark.parametrize("recompute", [0, 1])
def test_a_training_plan_is_refused(recompute):
    h = make_plan(inference=0, recompute=recompute)
    try:
        rc, err = tail(h)
        assert rc != 0 and "inference" in err
    finally:
        L.lib().lnx_plan_destroy(h)


def test_a_plan_without_metadata_components_is_refused():
    h = make_plan(n_meta=0)
    try:
        rc, err = tail(h)
        assert rc != 0 and "metadata" in err
    finally:
        L.lib().lnx_plan_destroy(h)


def test_null_meta_and_null_logits_are_refused():
    h = make_plan()
    h0 = make_plan(n_tasks=0)
    try:
        rc, err = tail(h, meta=None)
        assert rc != 0 and "NULL" in err and "meta" in err
        rc, err = tail(h, logits=None)
        assert rc != 0 and "NULL" in err and "logits" in err
        rc, err = tail(h0, logits=None)  # no tasks: logits may be NULL, the refusal is the next one in line
        assert rc != 0 and "NULL" not in err and "bound" in err
    finally:
        L.lib().lnx_plan_destroy(h)
        L.lib().lnx_plan_destroy(h0)


# ---------------------------------------------------------------------------------------------------------------- collate helpers
def test_variant_phase_names_are_the_references():
    combos = [(), None, ["TEMPORAL"], ["SPATIAL", "ELEVATION"]]
    assert collate.variant_phase_names(combos) == ["val", "val_mask_meta", "val_mask_TEMPORAL", "val_mask_SPATIAL_ELEVATION"]
    assert collate.variant_phase_names([None, []]) == ["val_mask_meta", "val"]


def test_variant_phase_names_refuse_what_is_no_list_of_combos():
    with pytest.raises(ValueError):
        collate.variant_phase_names([])
    with pytest.raises(ValueError):
        collate.variant_phase_names([(), []])  # the same phase twice
    with pytest.raises(TypeError):
        collate.variant_phase_names("TEMPORAL")
    with pytest.raises(TypeError):
        collate.variant_phase_names(["TEMPORAL"])  # a component name where a combo belongs
    with pytest.raises(TypeError):
        collate.variant_phase_names(None)


def test_meta_variants_checks_its_arguments_before_any_launch():
    aux = torch.zeros(3, 15)
    with pytest.raises(KeyError):
        collate.meta_variants(aux, BOUNDS, [(), ["ALTITUDE"]])
    with pytest.raises(ValueError):
        collate.meta_variants(aux, BOUNDS, [])
    with pytest.raises(ValueError):
        collate.meta_variants(torch.zeros(15), BOUNDS, [()])
    with pytest.raises(L.LnxError):  # host tensors: the masking runs on the device only
        collate.meta_variants(aux, BOUNDS, [(), None])
