"""The rotate mode of the RoPE attention (MODEL.ROPE_STAGES.ROPE_ROTATE / LNX_ROPE_ROTATE) without a GPU: the fp64 restatement
tests/rope_rotate_ref.py against what the reference's own helpers compute from the complex table (rope_rotate_ops.npz, recorded by
tests/golden/gen/make_golden_rope_rotate.py) and against torch's fp64 autograd through complex operations; the new pieces of the C
ABI; the configuration switch."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from oracle import mformer_oracle as O
from tests import rope_rotate_ref as RR
from tests.cases import CASES, make_config


def _ops(golden_dir):
    z = np.load(os.path.join(golden_dir, "rope_rotate_ops.npz"), allow_pickle=False)
    for i in range(int(z["n_cases"])):
        yield i, tuple(int(v) for v in z["cases"][i]), {k[: -len(f"_{i}")]: torch.from_numpy(z[k]) for k in z.files if k.endswith(f"_{i}")}


def test_restatement_reproduces_the_reference_helpers(golden_dir):
    """tables == compute_mixed_cis's complex table, rotate == apply_rotary_emb with it (both fp32 in the reference: a few ulp of
    values of size <= 8), and the cos-only form is the real part of the same table."""
    seen = 0
    for i, (heads, D, H, W, E), r in _ops(golden_dir):
        cos, sin = RR.tables(r["freqs"], H, W)
        torch.testing.assert_close(cos, r["cis_re"].double(), rtol=0, atol=2e-6)
        torch.testing.assert_close(sin, r["cis_im"].double(), rtol=0, atol=2e-6)
        torch.testing.assert_close(cos.float(), O.rope_cos_table(r["freqs"], H, W), rtol=0, atol=2e-6)  # the cos mode's table
        for x, want in (("q", "q_out"), ("k", "k_out")):
            torch.testing.assert_close(RR.rotate(r[x].double(), cos, sin), r[want].double(), rtol=1e-5, atol=1e-5)
        seen += 1
    assert seen >= 4
    assert any(H != W for _, (_, _, H, W, _), _ in _ops(golden_dir))


def test_rotation_backward_reproduces_the_recorded_fp64_gradients(golden_dir):
    for i, (heads, D, H, W, E), r in _ops(golden_dir):
        cos, sin = RR.tables(r["freqs"], H, W)
        torch.testing.assert_close(RR.rotate_bwd(r["wq"].double(), cos, sin), r["gq"], rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(RR.rotate_bwd(r["wk"].double(), cos, sin), r["gk"], rtol=1e-12, atol=1e-12)
        dth = RR.dtheta_of(r["wq"].double(), RR.rotate(r["q"].double(), cos, sin)) + RR.dtheta_of(r["wk"].double(), RR.rotate(r["k"].double(), cos, sin))
        torch.testing.assert_close(RR.dfreqs_of(dth, H, W), r["gf"], rtol=1e-10, atol=1e-10)


def _complex_attention(qkv, freqs, B, N, E, heads, hd, H, W, drop=None):
    """the rotated attention with torch complex operations (what apply_rotary_emb does), differentiable in fp64"""
    t = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    n = torch.arange(H * W, dtype=torch.float64)
    ang = (n % W)[:, None, None] * freqs[0][None] + torch.div(n, W, rounding_mode="floor")[:, None, None] * freqs[1][None]
    cis = torch.polar(torch.ones_like(ang), ang).permute(1, 0, 2)[None]
    rot = lambda x: torch.view_as_real(torch.view_as_complex(x.reshape(B, heads, H * W, hd // 2, 2).contiguous()) * cis).flatten(-2)  # noqa: E731
    q = torch.cat([q[:, :, :E], rot(q[:, :, E:])], 2) * hd ** -0.5
    k = torch.cat([k[:, :, :E], rot(k[:, :, E:])], 2)
    a = torch.softmax(q @ k.transpose(-2, -1), -1)
    if drop is not None:
        a = a * drop
    return (a @ v).transpose(1, 2).reshape(B * N, heads * hd)


@pytest.mark.parametrize("B,heads,hd,H,W,E,drop", [(2, 2, 32, 3, 5, 3, False), (1, 3, 64, 4, 6, 1, True), (2, 1, 128, 5, 2, 4, False), (1, 2, 64, 2, 2, 0, False)])
def test_handwritten_backward_equals_fp64_autograd_through_complex_ops(B, heads, hd, H, W, E, drop):
    N = H * W + E
    gen = torch.Generator().manual_seed(17 + hd + N)
    qkv = torch.randn(B * N, 3 * heads * hd, generator=gen, dtype=torch.float64).requires_grad_(True)
    freqs = (0.3 * torch.randn(2, heads, hd // 2, generator=gen, dtype=torch.float64)).requires_grad_(True)
    d_o = torch.randn(B * N, heads * hd, generator=gen, dtype=torch.float64)
    keep = ((torch.rand(B, heads, N, N, generator=gen) >= 0.25).double() / 0.75) if drop else None
    ref = _complex_attention(qkv, freqs, B, N, E, heads, hd, H, W, keep)
    ref.backward(d_o)
    o, saved = RR.attn_fwd(qkv.detach(), freqs.detach(), B, N, E, heads, hd, H, W, keep)
    torch.testing.assert_close(o, ref.detach(), rtol=1e-12, atol=1e-12)
    dqkv, dfreqs = RR.attn_bwd(d_o, saved, B, N, E, heads, hd, H, W)
    torch.testing.assert_close(dqkv, qkv.grad, rtol=1e-10, atol=1e-11)
    torch.testing.assert_close(dfreqs, freqs.grad, rtol=1e-10, atol=1e-10)


def test_cos_form_of_the_restatement_is_the_existing_fp64_reference():
    from tests.test_gpu_headdim import attn_ref

    B, heads, hd, H, W, E = 2, 2, 32, 3, 5, 3
    N = H * W + E
    gen = torch.Generator().manual_seed(5)
    qkv = torch.randn(B * N, 3 * heads * hd, generator=gen, dtype=torch.float64)
    freqs = 0.3 * torch.randn(2, heads, hd // 2, generator=gen, dtype=torch.float64)
    o, _ = RR.attn_fwd(qkv, freqs, B, N, E, heads, hd, H, W, rotate_mode=False)
    torch.testing.assert_close(o, attn_ref(qkv, freqs, B, N, E, heads, hd, H, W), rtol=1e-12, atol=1e-12)
    o_rot, _ = RR.attn_fwd(qkv, freqs, B, N, E, heads, hd, H, W)
    assert (o_rot - o).abs().max().item() > 1e-3  # the two modes are different functions


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_mode_constants_and_appended_fields():
    assert (L.ROPE_COS, L.ROPE_ROTATE) == (0, 1)
    from linnaeus_amd.model import _Cfg

    def names(cls):
        return [f[0] for f in cls._fields_]

    assert names(L.AttnArgs)[-2:] == ["rope_mode", "sin_tab"]
    assert names(L.AttnBwdArgs)[-3:] == ["rope_mode", "sin_tab", "grid_w"]
    assert names(L.RopeTable)[-2:] == ["rope_mode", "sin_out"]
    assert names(_Cfg)[-1] == "rope_mode"
    for cls in (L.AttnArgs, L.AttnBwdArgs, L.RopeTable, _Cfg):  # zero-initialised = the cos mode: existing callers are unaffected
        assert cls().rope_mode == L.ROPE_COS


def test_new_symbols_exported_and_version_bumped():
    lib = L.lib()
    assert "lnx_rope_cossin_table_hd" in L.EXPORTS and hasattr(lib, "lnx_rope_cossin_table_hd")
    assert lib.lnx_version() >= 103


def test_bad_rope_mode_is_refused_before_any_launch():
    lib = L.lib()
    fake = C.c_void_p(0x1000)
    a = L.AttnArgs()
    a.dtype, a.B, a.N, a.E, a.heads, a.qkv, a.o, a.cos_tab, a.rope_mode = L.BF16, 1, 8, 0, 1, fake, fake, fake, 2
    assert lib.lnx_attn_fwd(C.byref(a), None) != 0 and b"rope_mode" in lib.lnx_last_error()
    a.rope_mode = L.ROPE_ROTATE  # rotate without its sin table
    assert lib.lnx_attn_fwd(C.byref(a), None) != 0 and b"sin table" in lib.lnx_last_error()
    t = L.RopeTable()
    t.freqs, t.cos_out, t.heads, t.H, t.W, t.rope_mode = fake, fake, 1, 2, 2, L.ROPE_ROTATE
    assert lib.lnx_rope_cos_tables(C.byref(t), 1, None) != 0 and b"sin_out" in lib.lnx_last_error()


def test_dispatch_does_not_look_at_the_mode(monkeypatch):
    """lnx_attn_dispatch keeps its signature and its answers for every argument set the boundary tests enumerate"""
    from tests import test_gpu_attention_boundaries as TB

    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    lib = L.lib()
    n = 0
    for (dtype, hd), _ in TB.FAMILY.items():
        for N in TB.NS:
            assert lib.lnx_attn_dispatch(dtype, N, hd, 0) == TB.family_of(TB.FAMILY, dtype, hd, N), (dtype, hd, N)
            assert lib.lnx_attn_dispatch(dtype, N, hd, 1) == TB.family_of(TB.FAMILY_DROP, dtype, hd, N), (dtype, hd, N)
            n += 2
    assert n == 2 * 6 * len(TB.NS)


def test_plan_accepts_the_mode_and_keeps_its_parameters():
    from linnaeus_amd.model import _Cfg

    lib = L.lib()
    lib.lnx_plan_param_name.restype = C.c_char_p
    lib.lnx_plan_param_numel.restype = C.c_int64
    lib.lnx_plan_workspace_bytes.restype = C.c_int64
    got = {}
    for mode in (L.ROPE_COS, L.ROPE_ROTATE):
        for inference in (0, 1):
            cfg = _Cfg()
            cfg.dtype, cfg.batch, cfg.img_h, cfg.img_w, cfg.in_chans = L.BF16, 2, 64, 64, 3
            cfg.dims[:] = [32, 64, 128, 256]
            cfg.conv_depths[:] = [1, 1]
            cfg.rope_depths[:] = [1, 1]
            cfg.rope_heads[:] = [2, 4]
            cfg.mlp_hidden[:] = [512, 1024]
            cfg.inference, cfg.rope_mode = inference, mode
            h = C.c_void_p()
            assert lib.lnx_plan_create(C.byref(cfg), C.byref(h)) == 0, lib.lnx_last_error()
            n = lib.lnx_plan_num_params(h)
            got[(mode, inference)] = ([(lib.lnx_plan_param_name(h, i), lib.lnx_plan_param_numel(h, i)) for i in range(n)], lib.lnx_plan_workspace_bytes(h))
            lib.lnx_plan_destroy(h)
    assert got[(0, 0)][0] == got[(1, 0)][0] == got[(1, 1)][0]
    assert got[(1, 0)][1] <= got[(0, 0)][1]  # the sin table sits where the (twice as large) d-cos table was: no new workspace
    cfg.rope_mode = 5
    assert lib.lnx_plan_create(C.byref(cfg), C.byref(h)) != 0 and b"rope_mode" in lib.lnx_last_error()


# ---- configuration ------------------------------------------------------------------------------------------------------------------
HEADS = {"tiny_hd32": (4, 8), "tiny_hd128": (1, 2)}


def _model(spec, rotate):
    cfg = make_config(spec, 64)
    if rotate is not None:
        cfg.MODEL.ROPE_STAGES.ROPE_ROTATE = rotate
    return build_model(cfg, num_classes={t: c for t, c in spec.heads})


def test_switch_is_read_at_construction_and_tolerates_its_absence(golden_dir):
    a = CASES["tiny_a"]
    absent, off, on = _model(a, None), _model(a, False), _model(a, True)
    assert "ROPE_ROTATE" not in make_config(a, 64).MODEL.ROPE_STAGES
    assert absent.rope_rotate is False and off.rope_rotate is False and on.rope_rotate is True
    assert absent._make_cfg(2, 64, 64, True).rope_mode == L.ROPE_COS and on._make_cfg(2, 64, 64, True).rope_mode == L.ROPE_ROTATE
    assert on._make_cfg(2, 64, 64, False).rope_mode == L.ROPE_ROTATE
    shapes = lambda m: [(k, tuple(v.shape)) for k, v in m.state_dict().items()]  # noqa: E731
    assert shapes(absent) == shapes(off) == shapes(on)
    with open(os.path.join(golden_dir, "tiny_headdim_params.json")) as fh:
        ref = json.load(fh)
    for name, heads in HEADS.items():
        spec = O.Spec(conv_dims=a.conv_dims, conv_depths=a.conv_depths, rope_depths=a.rope_depths, rope_heads=heads, heads=a.heads)
        m = _model(spec, True)
        assert [[k, list(s)] for k, s in shapes(m)] == ref[name], name
        f = dict(shapes(m))["stages.2.0.attn.freqs"]
        assert f == (2, heads[0], 128 // heads[0] // 2)


def test_axial_rope_stays_refused_in_either_mode():
    cfg = make_config(CASES["tiny_a"], 64)
    cfg.MODEL.ROPE_STAGES.ROPE_MIXED = False
    cfg.MODEL.ROPE_STAGES.ROPE_ROTATE = True
    with pytest.raises(NotImplementedError):
        build_model(cfg, num_classes={t: c for t, c in CASES["tiny_a"].heads})
