"""Fine-tuning plans on the host (no GPU): the unit list and the parameter -> unit map of the planner, the freeze helpers of the
module, and the workspace of every cut (lnx_plan_create and lnx_plan_set_trainable need no device)."""
import ctypes as C

import pytest

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from oracle import mformer_oracle as O
from tests.cases import CASES, make_config

IMG = {"tiny_b": 96, "tiny_dp": 64, "sm": 224}


LG = O.Spec(conv_dims=(192, 384, 768, 1536), conv_depths=(3, 3), rope_depths=(9, 3), rope_heads=(12, 24), heads=(("taxa_L10", 100), ("taxa_L20", 10)))


def _model(name):
    spec = CASES[name]
    return build_model(make_config(spec, IMG[name]), num_classes={t: c for t, c in spec.heads})


def _lg():  # the large variant's depths and widths: more blocks per stage than sm
    return build_model(make_config(LG, 384), num_classes={t: c for t, c in LG.heads})


def _expected_units(depths, rdepths):
    a, b = depths[:2]
    c, d = rdepths
    return (["stem"] + [f"stages.0.{i}" for i in range(a)] + ["downsample_layers.0"] + [f"stages.1.{i}" for i in range(b)] +
            ["downsample_layers.1", "tokens_1"] + [f"stages.2.{i}" for i in range(c)] + ["mid", "tokens_2"] +
            [f"stages.3.{i}" for i in range(d)] + ["tail", "heads"])


def _expected_unit_of(name):
    """The issue's unit of a PLAN parameter name, restated from the name alone."""
    p = name.split(".")
    if p[0] == "stem":
        return "stem"
    if p[0] == "stages":
        return f"stages.{p[1]}.{p[2]}"
    if p[0] == "downsample_layers":
        return "mid" if p[1] == "2" else f"downsample_layers.{p[1]}"
    if p[0] in ("cls_token_1", "cls_token_2"):
        return "tokens_" + p[0][-1]
    if p[0] == "meta":
        return "tokens_" + p[2][-1]
    if p[0] in ("norm_1", "cl_1_fc"):
        return "mid"
    if p[0] in ("norm_2", "aggregate", "final_norm"):
        return "tail"
    assert p[0] == "head", name
    return "heads"


@pytest.mark.parametrize("which", ["sm", "lg", "tiny_b"])
def test_units_cover_every_parameter_once(which):
    model = _lg() if which == "lg" else _model(which)
    info = model.plan_units()
    assert info["units"] == _expected_units(model._depths, model._rdepths)
    layout = model.grad_arena_layout()
    assert info["names"] == layout["names"]  # every name of the arena layout, once, in plan order
    assert len(set(info["names"])) == len(info["names"]) == len(info["unit_of"])
    for nm, u in zip(info["names"], info["unit_of"]):
        assert 0 <= u < len(info["units"])
        assert info["units"][u] == _expected_unit_of(nm), nm
    used = {info["units"][u] for u in info["unit_of"]}
    assert used == set(info["units"])  # (these three have tasks: no unit is empty)


def _pattern(model):
    info = model.plan_units()
    on = set()
    for p_, u in zip(info["params"], info["unit_of"]):
        on.add((info["units"][u], p_.requires_grad))
    assert len({u for u, _ in on}) == len(on), "a unit with both frozen and trainable parameters"
    return {u for u, t in on if t}


def test_freeze_through_sets_the_pattern():
    model = _model("sm")
    units = model.plan_units()["units"]
    for name in ("stem", "stages.0.2", "tokens_1", "mid", "stages.3.0", "heads"):
        model.freeze_through(name)
        assert _pattern(model) == set(units[units.index(name):]), name
        assert model.trainable_report()["cut"] == name
        assert model.trainable_report()["backward_units"] == len(units) - units.index(name)
    with pytest.raises(ValueError):
        model.freeze_through("stages.9.0")
    model.freeze_through("stem")
    assert all(p_.requires_grad for p_ in model.parameters())


def test_unfreeze_last_blocks_is_the_phase_two_rule():
    model = _model("sm")  # 3 + 3 + 5 + 2 = 13 blocks
    units = model.plan_units()["units"]
    blocks = [u for u in units if u.startswith("stages.")]
    assert len(blocks) == 13
    model.unfreeze_last_blocks(0)
    assert _pattern(model) == {"tail", "heads"}
    model.unfreeze_last_blocks(1)
    assert _pattern(model) == {"stages.3.1", "tail", "heads"}
    assert model.trainable_report()["cut"] == "stages.3.1"
    model.unfreeze_last_blocks(3)  # the first unfrozen block is stages.2.4: mid and tokens_2 follow it
    assert _pattern(model) == {"stages.2.4", "mid", "tokens_2", "stages.3.0", "stages.3.1", "tail", "heads"}
    model.unfreeze_last_blocks(13)  # every block, and what follows the first: the stem and the ConvNeXt downsamplers stay frozen
    assert _pattern(model) == set(units) - {"stem", "downsample_layers.0", "downsample_layers.1"}
    assert model.trainable_report()["cut"] == "stages.0.0"
    model.unfreeze_last_blocks(14)
    assert _pattern(model) == set(units)
    assert all(p_.requires_grad for p_ in model.parameters())


def _c_queries(model, batch, img, mask):
    lib = L.lib()
    lib.lnx_plan_workspace_bytes.restype = C.c_int64
    cfg = model._make_cfg(batch, img, img, True, False)
    h = C.c_void_p()
    L.check(lib.lnx_plan_create(C.byref(cfg), C.byref(h)), "lnx_plan_create")
    try:
        base = int(lib.lnx_plan_workspace_bytes(h))
        if mask is not None:
            L.check(lib.lnx_plan_set_trainable(h, mask), "lnx_plan_set_trainable")
        return base, int(lib.lnx_plan_workspace_bytes(h)), lib.lnx_plan_first_trained_unit(h), lib.lnx_plan_num_units(h)
    finally:
        lib.lnx_plan_destroy(h)


@pytest.mark.parametrize("name,batch", [("sm", 8), ("tiny_dp", 2)])
def test_footprint_over_every_cut(name, batch, monkeypatch):
    model = _model(name)
    img = IMG[name]
    units = model.plan_units()["units"]
    full = model.workspace_bytes(batch, img)
    monkeypatch.setenv("LNX_FROZEN_PREFIX", "0")  # the planner without the feature: the figure of the parent for this shape
    parent = model.workspace_bytes(batch, img)
    model.freeze_through("heads")
    assert model.workspace_bytes(batch, img) == parent  # ... whatever is frozen
    assert model.trainable_report(batch, img)["cut"] == "stem"
    monkeypatch.delenv("LNX_FROZEN_PREFIX")
    model.freeze_through("stem")
    assert full == parent
    ws = {}
    for u in units:
        model.freeze_through(u)
        ws[u] = model.workspace_bytes(batch, img)
        rep = model.trainable_report(batch, img)
        mask = model._trainable_mask()
        base, got, cut, n_units = _c_queries(model, batch, img, mask)
        assert base == full - 256  # (workspace_bytes adds the alignment slack)
        assert rep == {"cut": u, "backward_units": n_units - cut, "workspace": got + 256}, u
        assert units[cut] == u and ws[u] == got + 256
    seq = [ws[u] for u in units]
    assert seq[0] == full
    assert all(b <= a for a, b in zip(seq, seq[1:])), list(zip(units, seq))
    assert ws["tokens_1"] < ws["stem"]
    assert ws["heads"] < ws["stages.3.0"]
    # another state than the current one, by parameter names; the current one is not changed by asking
    model.freeze_through("stem")
    names = [nm for nm, _ in model.named_parameters() if nm.startswith("head.")]
    assert model.workspace_bytes(batch, img, trainable=names) == ws["heads"]
    assert model.workspace_bytes(batch, img) == full
    # recompute plans shrink with the cut as well, and never exceed the kept-activation plan of the same cut
    for u in units:
        model.freeze_through(u)
        assert model.workspace_bytes(batch, img, recompute=True) <= ws[u], u


def test_autobatch_sees_the_smaller_plan():
    from linnaeus_amd.autobatch import predicted_bytes

    model = _model("sm")
    full = predicted_bytes(model, 64, 224, mode="train")
    model.freeze_through("heads")
    probe = predicted_bytes(model, 64, 224, mode="train")
    assert probe < full
    assert full - probe >= model.workspace_bytes(64, 224, trainable=[n for n, _ in model.named_parameters()]) - model.workspace_bytes(64, 224)


def test_set_trainable_refusals_on_the_host():
    model = _model("tiny_dp")
    lib = L.lib()
    n = len(model.plan_units()["names"])
    for train, mask, word in ((True, None, "NULL"), (True, bytes(n), "all zero"), (False, b"\x01" * n, "inference")):
        cfg = model._make_cfg(2, 64, 64, train, False)
        h = C.c_void_p()
        L.check(lib.lnx_plan_create(C.byref(cfg), C.byref(h)), "lnx_plan_create")
        try:
            assert lib.lnx_plan_set_trainable(h, mask) != 0
            assert word in lib.lnx_last_error().decode()
        finally:
            lib.lnx_plan_destroy(h)
    base, got, cut, _ = _c_queries(model, 2, 64, b"\x01" * n)
    assert base == got and cut == 0
