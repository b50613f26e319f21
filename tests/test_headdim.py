"""Attention head_dim 32 and 128 on the host side (no GPU): the planner and the nn.Module accept them, enumerate the reference's
parameters (attn.freqs = [2, heads, head_dim / 2]) and size their buffers by them; every other head_dim is refused by name."""
import ctypes as C
import json
import os

import pytest

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from oracle import mformer_oracle as O
from tests.cases import CASES, make_config

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HEADS = {"tiny_hd32": (4, 8), "tiny_hd128": (1, 2)}


def tiny_spec(rope_heads):
    a = CASES["tiny_a"]
    return O.Spec(conv_dims=a.conv_dims, conv_depths=a.conv_depths, rope_depths=a.rope_depths, rope_heads=rope_heads, heads=a.heads)


def make(rope_heads, **kw):
    spec = tiny_spec(rope_heads)
    return build_model(make_config(spec, 64), num_classes={t: c for t, c in spec.heads}, **kw)


def plan_params(model, batch=2):
    """(name, numel) of the native plan's parameter enumeration"""
    lib = L.lib()
    lib.lnx_plan_param_name.restype = C.c_char_p
    lib.lnx_plan_param_numel.restype = C.c_int64
    cfg = model._make_cfg(batch, 64, 64, True)
    h = C.c_void_p()
    assert lib.lnx_plan_create(C.byref(cfg), C.byref(h)) == 0, lib.lnx_last_error()
    try:
        return [(lib.lnx_plan_param_name(h, i).decode(), int(lib.lnx_plan_param_numel(h, i))) for i in range(lib.lnx_plan_num_params(h))]
    finally:
        lib.lnx_plan_destroy(h)


@pytest.mark.parametrize("name", ["tiny_hd32", "tiny_hd128"])
def test_plan_and_module_enumerate_the_reference_parameters(name):
    ref = json.load(open(os.path.join(GOLDEN, "tiny_headdim_params.json")))[name]
    model = make(HEADS[name])
    sd = model.state_dict()
    assert [k for k, _ in ref] == list(sd.keys())
    for k, shape in ref:
        assert list(sd[k].shape) == shape, (k, list(sd[k].shape), shape)
    hd = [d // h for d, h in zip(CASES["tiny_a"].conv_dims[2:], HEADS[name])]
    for s, h in enumerate(HEADS[name]):
        assert list(sd[f"stages.{s + 2}.0.attn.freqs"].shape) == [2, h, hd[s] // 2]
    # the native plan: the reference's numels in state_dict order, and its names (the plan calls the metadata heads
    # "meta.<index>.head_<stage>.*" and the classifiers "head.<task index>.*"; the module maps them onto the reference's names)
    got = plan_params(model)
    assert len(got) == len(ref)
    for (k, n), (rk, shape) in zip(got, ref):
        want = 1
        for v in shape:
            want *= v
        assert n == want, (k, rk, n, want)
        if not k.startswith(("meta.", "head.")):
            assert k == rk, (k, rk)


@pytest.mark.parametrize("rope_heads,hd", [((4, 8), 32), ((1, 2), 128), ((2, 2), None)])
def test_plan_create_through_the_c_abi(rope_heads, hd):
    """The C ABI directly (as test_abi.test_plan_create_validates_and_enumerates_parameters does for head_dim 64)."""
    from linnaeus_amd.model import _Cfg

    lib = L.lib()
    lib.lnx_plan_workspace_bytes.restype = C.c_int64
    cfg = _Cfg()
    cfg.dtype, cfg.batch, cfg.img_h, cfg.img_w, cfg.in_chans = L.BF16, 2, 64, 64, 3
    cfg.dims[:] = [32, 64, 128, 256]
    cfg.conv_depths[:] = [1, 1]
    cfg.rope_depths[:] = [1, 1]
    cfg.rope_heads[:] = list(rope_heads)
    cfg.mlp_hidden[:] = [512, 1024]
    cfg.n_meta, cfg.n_tasks = 0, 0
    h = C.c_void_p()
    assert lib.lnx_plan_create(C.byref(cfg), C.byref(h)) == 0, lib.lnx_last_error()
    lib.lnx_plan_param_name.restype = C.c_char_p
    lib.lnx_plan_param_numel.restype = C.c_int64
    freqs = {lib.lnx_plan_param_name(h, i).decode(): lib.lnx_plan_param_numel(h, i) for i in range(lib.lnx_plan_num_params(h))}
    assert freqs["stages.2.0.attn.freqs"] == 128 and freqs["stages.3.0.attn.freqs"] == 256  # 2 * heads * head_dim / 2 = dim
    assert lib.lnx_plan_workspace_bytes(h) > 0
    lib.lnx_plan_destroy(h)


@pytest.mark.parametrize("dims,rope_heads", [((96, 192), (2, 4)), ((192, 384), (4, 4)), ((128, 256), (3, 4)), ((128, 256), (2, 3))])
def test_other_head_dims_are_refused_by_name(dims, rope_heads):
    """head_dim 48, 96 and a non-integer split: refused by the planner and by the model, with head_dim in the message."""
    from linnaeus_amd.model import _Cfg

    lib = L.lib()
    cfg = _Cfg()
    cfg.dtype, cfg.batch, cfg.img_h, cfg.img_w, cfg.in_chans = L.BF16, 2, 64, 64, 3
    cfg.dims[:] = [32, 64, dims[0], dims[1]]
    cfg.conv_depths[:] = [1, 1]
    cfg.rope_depths[:] = [1, 1]
    cfg.rope_heads[:] = list(rope_heads)
    cfg.mlp_hidden[:] = [4 * dims[0], 4 * dims[1]]
    h = C.c_void_p()
    assert lib.lnx_plan_create(C.byref(cfg), C.byref(h)) != 0
    msg = lib.lnx_last_error()
    assert b"head_dim" in msg and b"32, 64 or 128" in msg, msg
    a = CASES["tiny_a"]
    spec = O.Spec(conv_dims=(32, 64) + tuple(dims), conv_depths=a.conv_depths, rope_depths=a.rope_depths, rope_heads=rope_heads, heads=a.heads)
    with pytest.raises(NotImplementedError, match="head_dim 32, 64 or 128"):
        build_model(make_config(spec, 64), num_classes={t: c for t, c in spec.heads})


def test_attention_entry_points_validate_head_dim_without_gpu():
    lib = L.lib()
    lib.lnx_attn_bwd_ws_floats_hd.restype = C.c_int64
    lib.lnx_attn_bwd_ws_floats.restype = C.c_int64
    assert lib.lnx_attn_bwd_ws_floats_hd(2, 100, 3, 64) == lib.lnx_attn_bwd_ws_floats(2, 100, 3) == 2 * 3 * 2 * 64
    assert lib.lnx_attn_bwd_ws_floats_hd(2, 100, 3, 128) == 2 * 3 * 2 * 128
    assert lib.lnx_attn_bwd_ws_floats_hd(2, 100, 3, 48) == 0
    fake = C.c_void_p(0x1000)
    for hd in (48, 96, 16):
        a = L.AttnArgs()
        a.dtype, a.B, a.N, a.E, a.heads, a.head_dim = L.BF16, 2, 100, 100, 3, hd
        a.qkv, a.o = fake, fake
        assert lib.lnx_attn_fwd(C.byref(a), None) != 0
        assert b"head_dim" in lib.lnx_last_error()
        b = L.AttnBwdArgs()
        b.dtype, b.B, b.N, b.E, b.heads, b.head_dim = L.BF16, 2, 100, 100, 3, hd
        b.qkv, b.o, b.lse, b.d_o, b.dqkv, b.delta = fake, fake, fake, fake, fake, fake
        assert lib.lnx_attn_bwd(C.byref(b), None) != 0
        assert b"head_dim" in lib.lnx_last_error()
        assert lib.lnx_rope_cos_table_hd(fake, 3, hd, 4, 4, fake, None, None) != 0
        assert b"head_dim" in lib.lnx_last_error()
        t = (L.RopeTable * 1)()
        t[0].freqs, t[0].cos_out, t[0].heads, t[0].H, t[0].W, t[0].head_dim = fake, fake, 3, 4, 4, hd
        assert lib.lnx_rope_cos_tables(t, 1, None) != 0
        assert b"head_dim" in lib.lnx_last_error()


@pytest.mark.parametrize("rope_heads", [(4, 8), (1, 2), (4, 2), (2, 4)])
def test_workspace_and_footprint_follow_head_dim(rope_heads):
    """plan_footprint reports the planner's workspace for head_dim 32, 128, a mix of both and 64."""
    lib = L.lib()
    lib.lnx_plan_workspace_bytes.restype = C.c_int64
    model = make(rope_heads)
    fp = model.plan_footprint(2)
    cfg = model._make_cfg(2, 64, 64, True)
    h = C.c_void_p()
    assert lib.lnx_plan_create(C.byref(cfg), C.byref(h)) == 0, lib.lnx_last_error()
    try:
        assert fp["workspace"] == lib.lnx_plan_workspace_bytes(h) + 256
    finally:
        lib.lnx_plan_destroy(h)


def test_grad_arena_and_parameter_bookkeeping_follow_the_plan():
    """grad_arena_layout / the flat arena hold every parameter, freqs at [2, heads, head_dim / 2] included."""
    model = make((4, 2))
    lay = model.grad_arena_layout()
    total = sum(p.numel() for p in model.parameters())
    assert lay["total"] >= total
    assert tuple(model.state_dict()["stages.2.0.attn.freqs"].shape) == (2, 4, 16)
    assert tuple(model.state_dict()["stages.3.0.attn.freqs"].shape) == (2, 2, 64)
