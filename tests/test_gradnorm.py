"""GradNorm task weighting (LOSS.GRAD_WEIGHTING.TASK.TYPE = gradnorm) on the host: construction and the reference's state-dict
names, initial weights, backbone selection by EXCLUDE_CONFIG, the arena-slice descriptor table and the new ABI structs.
The device path is in tests/test_gpu_gradnorm.py."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from linnaeus_amd.config import ConfigNode
from linnaeus_amd.loss import (DEFAULT_EXCLUDE_CONFIG, GradientWeighting, GradNormModule, backbone_slices, gradnorm_desc_table, param_filter)
from tests.cases import CASES, make_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
TASKS = ["taxa_L10", "taxa_L20", "taxa_L30", "taxa_L40"]


def gradnorm_cfg(spec=None, img=64, **task):
    cfg = make_config(spec or CASES["tiny_a"], img)
    t = {"TYPE": "gradnorm", "ALPHA": 1.5, "ZERO_AUX_INFO": True, "GRADNORM_ACCUM_STEPS": 1, "EXCLUDE_CONFIG": DEFAULT_EXCLUDE_CONFIG}
    t.update(task)
    cfg.LOSS = ConfigNode({"GRAD_WEIGHTING": {"TASK": t}})
    cfg.TRAIN.GRADIENT_CHECKPOINTING.ENABLED_GRADNORM_STEPS = False
    return cfg


def test_gradnorm_is_constructed_with_the_reference_buffers():
    gw = GradientWeighting(TASKS, gradnorm_cfg(), "gradnorm")
    assert gw.gradnorm is not None and gw.task_weighting_type == "gradnorm"
    assert set(gw.state_dict().keys()) == {"gradnorm.task_weights", "gradnorm.initial_losses"}
    assert gw.gradnorm.task_weights.tolist() == [1.0] * 4 and gw.gradnorm.initial_losses.tolist() == [0.0] * 4
    assert gw.exclude_patterns == ["head", "meta_"] and gw.zero_aux_info is True and gw.keep_step_grads is False
    # a reference state dict loads (and ours is what the reference would load: same names, shapes, dtypes)
    ref = {"gradnorm.task_weights": torch.tensor([0.5, 1.5, 1.0, 1.0]), "gradnorm.initial_losses": torch.tensor([2.0, 3.0, 1.0, 4.0])}
    gw.load_state_dict(ref)
    assert gw.gradnorm.task_weights.tolist() == [0.5, 1.5, 1.0, 1.0]
    other = GradientWeighting(TASKS, gradnorm_cfg(), "gradnorm")
    other.load_state_dict(gw.state_dict())
    assert torch.equal(other.gradnorm.initial_losses, ref["gradnorm.initial_losses"])
    # the static path stays as it was; other types are refused
    assert GradientWeighting(TASKS, None, "static").gradnorm is None
    with pytest.raises(NotImplementedError):
        GradientWeighting(TASKS, None, "uncertainty")


def test_zero_aux_info_comes_from_the_config_first():
    assert GradientWeighting(TASKS, gradnorm_cfg(ZERO_AUX_INFO=False), "gradnorm", zero_aux_info=True).zero_aux_info is False


def test_initial_weights_follow_the_reference_rules():
    # GradientWeighting always hands GradNormModule a tensor: INIT_WEIGHTS or ones, label densities never take effect
    gw = GradientWeighting(TASKS, gradnorm_cfg(), "gradnorm", label_densities={"taxa_L10": 0.1, "taxa_L20": 0.5}, init_strategy="inverse_density")
    assert gw.gradnorm.task_weights.tolist() == [1.0] * 4
    gw = GradientWeighting(TASKS, gradnorm_cfg(), "gradnorm", init_weights={"taxa_L20": 2.0, "taxa_L40": 0.25})
    assert gw.gradnorm.task_weights.tolist() == [1.0, 2.0, 1.0, 0.25]
    gw = GradientWeighting(TASKS, gradnorm_cfg(), "gradnorm", init_weights=[3.0, 1.0, 1.0, 1.0])
    assert gw.gradnorm.task_weights.tolist() == [3.0, 1.0, 1.0, 1.0]
    # GradNormModule itself (init_weights None) computes them from the strategy, normalised to sum to T
    m = GradNormModule(["a", "b"], init_weights=None, label_densities={"a": 0.25, "b": 0.5})
    np.testing.assert_allclose(m.task_weights.numpy(), [4 / 3, 2 / 3], rtol=1e-6)
    m = GradNormModule(["a", "b"], init_weights=None, label_densities={"a": 0.5, "b": 0.5}, num_classes={"a": 10, "b": 100}, init_strategy="class_complexity")
    np.testing.assert_allclose(m.task_weights.numpy(), [2 * 0.5 / 1.5, 2 * 1.0 / 1.5], rtol=1e-6)
    assert GradNormModule(["a", "b"], init_weights=None).task_weights.tolist() == [1.0, 1.0]
    assert m.get_task_weights() == {"a": pytest.approx(2 / 3), "b": pytest.approx(4 / 3)}


def test_parameter_filters_follow_the_reference_config_language():
    p = torch.zeros(3, 3)
    f = param_filter(DEFAULT_EXCLUDE_CONFIG)
    assert f("head.taxa_L10.fc.weight", p) and f("meta_temporal_head_1.0.weight", p) and f("module.head.x", p)
    assert not f("stages.2.0.attn.qkv.weight", p)
    g = param_filter({"TYPE": "and", "FILTERS": [{"TYPE": "name", "PATTERNS": ["stages."], "MATCH_TYPE": "startswith"},
                                                  {"TYPE": "not", "FILTER": {"TYPE": "dimension", "DIMENSIONS": [1]}}]})
    assert g("stages.0.0.pwconv1.weight", p) and not g("stages.0.0.pwconv1.bias", torch.zeros(3)) and not g("stem.0.weight", p)
    assert param_filter({"TYPE": "name", "PATTERNS": [r"norm\d"], "MATCH_TYPE": "regex"})("stages.2.0.norm1.weight", p)
    with pytest.raises(ValueError):
        param_filter({"TYPE": "layer_type", "LAYER_TYPES": ["Linear"]})


def test_backbone_selection_matches_the_reference_on_sm():
    """set_model selects, in named_parameters order, exactly the parameters the reference's GradientWeighting.set_model picks on
    mFormerV1_sm with the default EXCLUDE_CONFIG (list recorded by tests/golden/gen/make_golden_gradnorm.py)."""
    want = json.load(open(os.path.join(GOLDEN, "gradnorm_backbone_sm.json")))
    spec = CASES["sm"]
    model = build_model(gradnorm_cfg(spec, 224), num_classes={t: c for t, c in spec.heads})
    gw = GradientWeighting([t for t, _ in spec.heads], gradnorm_cfg(spec, 224), "gradnorm")

    class Wrapped(torch.nn.Module):  # DDP-style wrapper: set_model unwraps .module
        def __init__(self, m):
            super().__init__()
            self.module = m

    gw.set_model(Wrapped(model))
    assert gw.backbone_names == want
    assert all(p is model.get_parameter(n) for p, n in zip(gw.backbone_params, want))


def test_backbone_descriptor_table_covers_the_backbone_slices_of_the_arena():
    spec = CASES["tiny_a"]
    model = build_model(gradnorm_cfg(spec), num_classes={t: c for t, c in spec.heads})
    gw = GradientWeighting([t for t, _ in spec.heads], gradnorm_cfg(spec), "gradnorm")
    gw.set_model(model)
    layout = model.grad_arena_layout()
    sl = backbone_slices(layout, gw.backbone_params)
    # every backbone parameter the plan differentiates appears once, at its own slice; no head / metadata slice is included
    by_id = {id(p): (o, n) for o, n, p in zip(layout["offsets"], layout["numels"], layout["params"])}
    assert sorted(by_id[id(p)] for p in gw.backbone_params if id(p) in by_id) == sl
    assert sum(n for _, n in sl) == sum(p.numel() for p in gw.backbone_params)
    heads = {id(p) for n, p in model.named_parameters() if n.startswith(("head.", "meta_"))}
    assert not any(by_id[i] in sl for i in heads if i in by_id)
    assert all(o % 4 == 0 and o + n <= layout["total"] for o, n in sl)
    for (o0, n0), (o1, _) in zip(sl, sl[1:]):
        assert o0 + n0 <= o1
    base = 1 << 20
    arr, blk = gradnorm_desc_table(sl, base)
    assert len(arr) == len(sl)
    acc = 0
    for d, (o, n) in zip(arr, sl):
        assert d.g == base + 4 * o and d.n == n and d.block_start == acc
        acc += L.lib().lnx_adamw_blocks(C.c_int64(n))
    assert blk == acc


def test_scratch_arenas_and_footprint():
    spec = CASES["tiny_a"]
    model = build_model(gradnorm_cfg(spec), num_classes={t: c for t, c in spec.heads})
    tasks = [t for t, _ in spec.heads]
    assert GradientWeighting(tasks, gradnorm_cfg(spec), "gradnorm").scratch_arenas() == 1
    assert GradientWeighting(tasks, gradnorm_cfg(spec, GRADNORM_ACCUM_STEPS=2), "gradnorm").scratch_arenas() == 2
    assert GradientWeighting(tasks, None, "static").scratch_arenas() == 0
    f0, f2 = model.plan_footprint(4, 64), model.plan_footprint(4, 64, gradnorm_arenas=2)
    assert "gradnorm" not in f0 and {k: v for k, v in f2.items() if k != "gradnorm"} == f0
    assert f2["gradnorm"] == 2 * 4 * model.grad_arena_layout()["total"] + f0["logits"] // 2


def test_gradnorm_args_mirror_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu\\n", sizeof(lnx_gradnorm_args), offsetof(lnx_gradnorm_args, norm), offsetof(lnx_gradnorm_args, metrics));\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    size, o_norm, o_metrics = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert (size, o_norm, o_metrics) == (C.sizeof(L.GradNormArgs), L.GradNormArgs.norm.offset, L.GradNormArgs.metrics.offset)


def test_gradnorm_entry_points_validate_without_a_gpu():
    lib = L.lib()
    a = L.GradNormArgs()
    a.T = 0
    assert lib.lnx_gradnorm_update(C.byref(a), None) != 0 and b"lnx_gradnorm_update" in lib.lnx_last_error()
    a.T = 17
    assert lib.lnx_gradnorm_update(C.byref(a), None) != 0
    fake = C.c_void_p(0x1000)
    assert lib.lnx_gradnorm_sumsq(fake, 1, 1, 17, 0, None, fake, fake, None) != 0 and b"ntasks" in lib.lnx_last_error()
    assert lib.lnx_gradnorm_sumsq(fake, 1, 1, 2, 0, None, fake, fake, None) != 0 and b"task_stride" in lib.lnx_last_error()
    assert lib.lnx_plan_backward_into(None, None, None, None, None) != 0 and b"lnx_plan_backward_into" in lib.lnx_last_error()


def test_fixture_was_recorded_with_the_cases_it_names():
    z = np.load(os.path.join(GOLDEN, "gradnorm.npz"), allow_pickle=False)
    from oracle import mformer_oracle as O
    from tests.cases import SEED

    for call in range(2):  # the images are regenerated from the seed: check they are the recorded ones
        x, _ = O.seeded_inputs(CASES["tiny_a"], 4, 64, SEED + 100 + call)
        assert float(x.double().sum()) == pytest.approx(float(z[f"x_sum_{call}"]), rel=1e-12)
    for c in ("c0", "c1", "c2"):
        assert list(z[f"{c}_0_metric_keys"])[0] == "gradnorm/avg_norm"
        np.testing.assert_allclose(z[f"{c}_1_weights"].sum(), 2.0, rtol=1e-6)


def test_autobatch_counts_the_gradnorm_scratch():
    from linnaeus_amd.autobatch import predicted_bytes

    spec = CASES["tiny_a"]
    model = build_model(gradnorm_cfg(spec), num_classes={t: c for t, c in spec.heads})
    assert predicted_bytes(model, 4, 64, gradnorm_arenas=1) - predicted_bytes(model, 4, 64) == model.plan_footprint(4, 64, gradnorm_arenas=1)["gradnorm"]
