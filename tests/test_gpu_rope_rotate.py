"""The rotate mode of the RoPE attention (MODEL.ROPE_STAGES.ROPE_ROTATE / LNX_ROPE_ROTATE) on the GPU.

Op level: lnx_attn_fwd / lnx_attn_bwd in rotate mode against the fp64 restatement tests/rope_rotate_ref.py (pinned to the reference's
helpers by tests/test_rope_rotate.py), on every kernel family, with the tolerances test_gpu_headdim.py / test_gpu_attention_boundaries.py
use for the same dtype (forward 3e-5 / 2e-2, dqkv and dfreqs 1e-4 / 4e-2 for fp32 / bf16: one rounding of the transformed operand in
either mode).  Exact invariants bit for bit.  Whole models against fixtures recorded from the reference with its cast removed
(tests/golden/gen/make_golden_rope_rotate.py), under test_gpu_headdim.py's bounds."""
import ctypes as C

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model, ops
from oracle import mformer_oracle as O
from tests import rope_rotate_ref as RR
from tests.cases import CASES, SEED, make_config, model_state_dict_from_oracle

pytestmark = pytest.mark.gpu
DT = {L.F32: torch.float32, L.BF16: torch.bfloat16}
DTN = {L.F32: "fp32", L.BF16: "bf16"}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
B, HEADS, RATE = 2, 2, 0.25
# (H, W, E): N = 50, 199, 260, 579, 1028 and the non-square 8 x 16 (N = 131).  bf16 head_dim 64 runs resident 4-wave, resident 8-wave,
# then the 128-row tiled kernels; bf16 head_dim 128 the 64-row ones at N = 50 and the 128-row ones beyond; fp32 and bf16 head_dim 32 the
# 64-row tiled kernels throughout
GRIDS = [(7, 7, 1), (14, 14, 3), (16, 16, 4), (24, 24, 3), (32, 32, 4), (8, 16, 3)]


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def run_op(qkv, d_o, freqs, H, W, E, hd, mode, mask=None, defer=False, nb=B, dfreqs=None):
    """forward + backward of one call on the GPU; mode 'rotate' or 'cos'.  Returns CPU copies and the families that ran."""
    N = H * W + E
    C_ = HEADS * hd
    dt = qkv.dtype
    cos = sin = dsin = None
    if H * W:
        if mode == "rotate":
            cos, sin = ops.rope_cossin_table(freqs, H, W)
        else:
            dsin = torch.empty(2, H * W, HEADS, hd // 2, device="cuda")
            cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
    o = torch.full((nb * N, C_), float("nan"), device="cuda", dtype=dt)
    lse = torch.full((nb, HEADS, N), float("nan"), device="cuda")
    dqkv = torch.full((nb * N, 3 * C_), float("nan"), device="cuda", dtype=dt)
    delta = torch.empty(nb, HEADS, N, device="cuda")
    if dfreqs is None:
        dfreqs = torch.zeros(2, HEADS, hd // 2, device="cuda")
    kw = {} if mask is None else dict(drop_mask=mask, drop_rate=RATE)
    rot = dict(sin_tab=sin) if mode == "rotate" and H * W else {}
    ops.attn_fwd(qkv, cos, o, lse, nb, N, E, HEADS, **kw, **rot)
    fam_f = L.lib().lnx_last_attn_kernel()
    if rot:
        rot["grid_w"] = W
    ws = ops.attn_bwd(qkv, cos, o, lse, d_o, dqkv, delta, nb, N, E, HEADS, dsin=dsin, dfreqs=dfreqs if H * W else None, defer_freqs=defer, **kw, **rot)
    fam_b = L.lib().lnx_last_attn_kernel()
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, dqkv=dqkv, dfreqs=dfreqs, families=(fam_f, fam_b), keep=(ws, cos, sin, dsin, delta))


def inputs(dtype, hd, H, W, E, seed, drop=False, nb=B):
    N = H * W + E
    gen = torch.Generator().manual_seed(seed + 1000 * N + hd + dtype)
    qkv = torch.randn(nb * N, 3 * HEADS * hd, generator=gen).to(DT[dtype])
    d_o = torch.randn(nb * N, HEADS * hd, generator=gen).to(DT[dtype])
    freqs = O.seeded_fill("t.attn.freqs", (2, HEADS, hd // 2), 7)
    mask = None
    if drop:
        mask = (torch.rand(nb, HEADS, N, (N + 63) // 64 * 64, generator=gen) >= RATE).to(torch.uint8)
    return qkv, d_o, freqs, mask


def check_against_fp64(dtype, hd, H, W, E, drop):
    N = H * W + E
    qkv, d_o, freqs, mask = inputs(dtype, hd, H, W, E, 3, drop)
    got = run_op(qkv.cuda(), d_o.cuda(), freqs.cuda(), H, W, E, hd, "rotate", None if mask is None else mask.cuda())
    want = L.lib().lnx_attn_dispatch(dtype, N, hd, int(drop))
    assert got["families"] == (want, want), (got["families"], want)
    keep = None if mask is None else mask[..., :N].double() / (1.0 - RATE)
    o, saved = RR.attn_fwd(qkv, freqs, B, N, E, HEADS, hd, H, W, keep)
    dqkv, dfreqs = RR.attn_bwd(d_o, saved, B, N, E, HEADS, hd, H, W)
    tol = 3e-5 if dtype == L.F32 else 2e-2
    tolb = 1e-4 if dtype == L.F32 else 4e-2
    err = lambda a, b: float((a.double().cpu() - b).abs().max())  # noqa: E731
    print(f"rotate {DTN[dtype]} hd{hd} {H}x{W}+{E} drop={int(drop)} family={want}: max err o {err(got['o'], o):.3e} dqkv {err(got['dqkv'], dqkv):.3e}"
          f" dfreqs {err(got['dfreqs'], dfreqs):.3e} of {float(dfreqs.abs().max()):.3e}")
    torch.testing.assert_close(got["o"].double().cpu(), o, rtol=tol, atol=tol)
    torch.testing.assert_close(got["dqkv"].double().cpu(), dqkv, rtol=tolb, atol=tolb)
    scale = dfreqs.abs().max().item()
    torch.testing.assert_close(got["dfreqs"].double().cpu(), dfreqs, rtol=tolb, atol=tolb * max(scale, 1.0))
    return want


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g_: "%dx%d+%d" % g_)
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=DTN.get)
def test_rotate_against_fp64(dtype, hd, grid, monkeypatch):
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    check_against_fp64(dtype, hd, *grid, False)


def test_every_family_is_in_the_grid(monkeypatch):
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    fams = {L.lib().lnx_attn_dispatch(dt, H * W + E, hd, 0) for dt in (L.F32, L.BF16) for hd in (32, 64, 128) for H, W, E in GRIDS}
    assert fams == {L.ATTN_KERNEL_RES4, L.ATTN_KERNEL_RES8, L.ATTN_KERNEL_TILED4, L.ATTN_KERNEL_TILED8}


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=DTN.get)
def test_rotate_with_attention_dropout_against_fp64(dtype, hd):
    assert check_against_fp64(dtype, hd, 14, 14, 3, True) == L.ATTN_KERNEL_TILED4  # the dropout-mask instantiations
    check_against_fp64(dtype, hd, 5, 9, 4, True)


@pytest.mark.parametrize("hd,dtype,H,W,E", [(64, L.BF16, 3, 4, 3), (64, L.F32, 2, 6, 4), (32, L.BF16, 3, 4, 1), (128, L.BF16, 2, 5, 3), (128, L.F32, 3, 3, 3)])
def test_deferred_fold_gives_the_bits_of_the_immediate_one(hd, dtype, H, W, E):
    """N <= 16: one wave's rows per workgroup carry image tokens, so the per-workgroup partials are the same bits in every run (beyond
    that the order of a workgroup's LDS adds varies from run to run, csrc/attention.hip freq_accum) and the two folds can be compared
    bit for bit."""
    qkv, d_o, freqs, _ = inputs(dtype, hd, H, W, E, 11)
    a = run_op(qkv.cuda(), d_o.cuda(), freqs.cuda(), H, W, E, hd, "rotate", dfreqs=torch.ones(2, HEADS, hd // 2, device="cuda"))
    b = run_op(qkv.cuda(), d_o.cuda(), freqs.cuda(), H, W, E, hd, "rotate", dfreqs=torch.ones(2, HEADS, hd // 2, device="cuda"), defer=True)
    assert bool((b["dfreqs"] == 1).all())  # nothing folded yet
    ops.attn_bwd_flush()
    torch.cuda.synchronize()
    assert not bool((a["dfreqs"] == 1).all())
    assert torch.equal(a["dfreqs"], b["dfreqs"])
    assert torch.equal(bits(a["dqkv"]), bits(b["dqkv"]))


@pytest.mark.parametrize("hd,dtype,H,W,E", [(64, L.BF16, 14, 14, 3), (64, L.BF16, 24, 24, 4), (32, L.F32, 8, 16, 3), (128, L.BF16, 16, 16, 4)])
def test_deferred_fold_on_multi_wave_shapes(hd, dtype, H, W, E):
    """the bound test_gpu_headdim.test_postponed_folds_of_mixed_head_dims applies between a postponed and an immediate fold"""
    qkv, d_o, freqs, _ = inputs(dtype, hd, H, W, E, 12)
    a = run_op(qkv.cuda(), d_o.cuda(), freqs.cuda(), H, W, E, hd, "rotate", dfreqs=torch.ones(2, HEADS, hd // 2, device="cuda"))
    b = run_op(qkv.cuda(), d_o.cuda(), freqs.cuda(), H, W, E, hd, "rotate", dfreqs=torch.ones(2, HEADS, hd // 2, device="cuda"), defer=True)
    ops.attn_bwd_flush()
    torch.cuda.synchronize()
    torch.testing.assert_close(b["dfreqs"], a["dfreqs"], rtol=1e-5, atol=1e-5 * float(a["dfreqs"].abs().max()))


# ---- exact invariants -------------------------------------------------------------------------------------------------------------
INV = [(hd, dt, g_) for hd in (32, 64, 128) for dt in (L.F32, L.BF16) for g_ in ((7, 7, 1), (14, 14, 3), (16, 16, 4), (8, 16, 3))]


@pytest.mark.parametrize("hd,dtype,grid", INV, ids=lambda v: DTN.get(v, str(v)) if isinstance(v, int) and v in DTN else str(v))
def test_zero_frequencies_make_the_two_modes_equal(hd, dtype, grid):
    """theta = 0: cos = 1, sin = 0, both modes leave q and k as they are -- o, lse and dqkv bit for bit (dfreqs differs by design: the
    cos mode's d cos / d freqs vanishes at theta = 0, the rotation's d theta does not)."""
    H, W, E = grid
    qkv, d_o, freqs, _ = inputs(dtype, hd, H, W, E, 21)
    z = torch.zeros_like(freqs).cuda()
    a = run_op(qkv.cuda(), d_o.cuda(), z, H, W, E, hd, "rotate")
    b = run_op(qkv.cuda(), d_o.cuda(), z, H, W, E, hd, "cos")
    assert a["families"] == b["families"]
    for k in ("o", "dqkv"):
        assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(a["lse"], b["lse"])
    assert bool((b["dfreqs"] == 0).all()) and float(a["dfreqs"].abs().max()) > 0


@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=DTN.get)
@pytest.mark.parametrize("N", [40, 131, 300])
def test_without_image_tokens_the_two_modes_are_equal(hd, dtype, N):
    qkv, d_o, freqs, _ = inputs(dtype, hd, 0, 0, N, 22)
    outs = []
    for mode in (L.ROPE_ROTATE, L.ROPE_COS):  # through the raw structs: E == N takes no tables in either mode
        q, d = qkv.cuda(), d_o.cuda()
        o = torch.full((B * N, HEADS * hd), float("nan"), device="cuda", dtype=DT[dtype])
        lse = torch.empty(B, HEADS, N, device="cuda")
        a = L.AttnArgs()
        a.dtype, a.B, a.N, a.E, a.heads, a.head_dim, a.rope_mode = dtype, B, N, N, HEADS, hd, mode
        a.qkv, a.o, a.lse = q.data_ptr(), o.data_ptr(), lse.data_ptr()
        L.check(L.lib().lnx_attn_fwd(C.byref(a), ops._stream()), "lnx_attn_fwd")
        dqkv = torch.full((B * N, 3 * HEADS * hd), float("nan"), device="cuda", dtype=DT[dtype])
        delta = torch.empty(B, HEADS, N, device="cuda")
        ba = L.AttnBwdArgs()
        ba.dtype, ba.B, ba.N, ba.E, ba.heads, ba.head_dim, ba.rope_mode = dtype, B, N, N, HEADS, hd, mode
        ba.qkv, ba.o, ba.lse, ba.d_o, ba.dqkv, ba.delta = q.data_ptr(), o.data_ptr(), lse.data_ptr(), d.data_ptr(), dqkv.data_ptr(), delta.data_ptr()
        L.check(L.lib().lnx_attn_bwd(C.byref(ba), ops._stream()), "lnx_attn_bwd")
        torch.cuda.synchronize()
        outs.append((o, lse, dqkv))
    assert not torch.isnan(outs[0][0].float()).any() and not torch.isnan(outs[0][2].float()).any()
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(bits(outs[0][2]), bits(outs[1][2]))


@pytest.mark.parametrize("hd,dtype,grid", [(64, L.BF16, (7, 7, 1)), (64, L.BF16, (14, 14, 3)), (64, L.BF16, (16, 16, 4)), (128, L.BF16, (8, 16, 3)),
                                           (32, L.BF16, (14, 14, 3)), (64, L.F32, (8, 16, 3)), (128, L.F32, (7, 7, 1)), (32, L.F32, (16, 16, 4))])
@pytest.mark.parametrize("drop", [False, True], ids=["plain", "drop"])
def test_nothing_outside_the_sequence_reaches_its_results(hd, dtype, grid, drop):
    """The sentinel style of test_gpu_attention_boundaries.py: sample 0's o, lse and dqkv do not change by one bit when sample 1 goes
    from ordinary values to |x| = 1e3 (and the mask's padding columns are flipped); the v rows are rotated in neither."""
    H, W, E = grid
    N = H * W + E
    qkv, d_o, freqs, mask = inputs(dtype, hd, H, W, E, 31, drop)
    gen = torch.Generator().manual_seed(99)
    big = lambda t: torch.where(torch.rand(t.shape, generator=gen) < 0.5, -1e3, 1e3).to(t.dtype)  # noqa: E731
    qkv2, d_o2 = qkv.clone(), d_o.clone()
    qkv2[N:], d_o2[N:] = big(qkv2[N:]), big(d_o2[N:])
    mask2 = None
    if drop:
        mask2 = mask.clone()
        mask2[..., N:] ^= 1
        mask2[1] ^= 1
    a = run_op(qkv.cuda(), d_o.cuda(), freqs.cuda(), H, W, E, hd, "rotate", None if mask is None else mask.cuda())
    b = run_op(qkv2.cuda(), d_o2.cuda(), freqs.cuda(), H, W, E, hd, "rotate", None if mask2 is None else mask2.cuda())
    for k in ("o", "dqkv"):
        assert not torch.isnan(a[k].float()).any(), k
        assert torch.equal(bits(a[k][:N]), bits(b[k][:N])), k
    assert torch.equal(a["lse"][0], b["lse"][0])
    # one sample alone gives sample 0's bits as well (nothing of sample 1 is needed)
    c = run_op(qkv[:N].cuda(), d_o[:N].cuda(), freqs.cuda(), H, W, E, hd, "rotate", None if mask is None else mask[:1].contiguous().cuda(), nb=1)
    assert torch.equal(bits(a["o"][:N]), bits(c["o"])) and torch.equal(bits(a["dqkv"][:N]), bits(c["dqkv"]))


def test_tables_batched_equal_single_and_match_fp64():
    heads, H, W = 3, 7, 9
    entries, want = [], []
    for i, d in enumerate([64, 32, 128, 64]):
        f = O.seeded_fill(f"t.rot.batch.{i}", (2, heads, d // 2), 9 + i).cuda()
        c1, s1 = ops.rope_cossin_table(f, H, W)
        rc, rs = RR.tables(f.cpu(), H, W)
        torch.testing.assert_close(c1.cpu().double(), rc, rtol=0, atol=2e-6)
        torch.testing.assert_close(s1.cpu().double(), rs, rtol=0, atol=2e-6)
        assert torch.equal(c1, ops.rope_cos_table(f, H, W))
        out = torch.full((H * W, heads, d // 2), float("nan"), device="cuda")
        sn = torch.full((H * W, heads, d // 2), float("nan"), device="cuda")
        rotate = i != 3  # the last entry stays a cos-mode table: modes mix in one call
        ds = None if rotate else torch.full((2, H * W, heads, d // 2), float("nan"), device="cuda")
        entries.append((f, H, W, out, ds, sn if rotate else None))
        want.append((c1, s1 if rotate else None))
    ops.rope_cos_tables(entries)
    torch.cuda.synchronize()
    for (_, _, _, out, ds, sn), (c1, s1) in zip(entries, want):
        assert torch.equal(out, c1)
        if sn is not None:
            assert torch.equal(sn, s1)
        else:
            assert not torch.isnan(ds).any()


# ---- whole model against the reference's fixtures ---------------------------------------------------------------------------------
MODEL_HEADS = {"tiny_rot_hd64": (2, 4), "tiny_rot_hd32": (4, 8), "tiny_rot_hd128": (1, 2)}


def load(name, golden_dir):
    a = CASES["tiny_a"]
    spec = O.Spec(conv_dims=a.conv_dims, conv_depths=a.conv_depths, rope_depths=a.rope_depths, rope_heads=MODEL_HEADS[name], heads=a.heads)
    z = np.load(f"{golden_dir}/{name}.npz", allow_pickle=False)
    sd = O.seeded_state_dict(O.param_shapes(spec), SEED)
    return spec, z, sd, torch.from_numpy(z["x"]), torch.from_numpy(z["meta"])


def build(spec, sd, dtype, rotate=True, img=64):
    cfg = make_config(spec, img)
    if rotate is not None:
        cfg.MODEL.ROPE_STAGES.ROPE_ROTATE = rotate
    model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype(dtype)
    return model


def grads_of(model):
    return {k: p_.grad.detach().clone() for k, p_ in model.named_parameters()}


@pytest.mark.parametrize("name", list(MODEL_HEADS))
def test_forward_fp32_matches_the_uncast_reference(name, golden_dir):
    """fp32 strict mode: the project's stated fp32 bound (rel 1e-4 / abs 1e-5), argmax exact; the inference plan's
    logits are the training plan's."""
    spec, z, sd, x, meta = load(name, golden_dir)
    model = build(spec, sd, "fp32")
    model.eval()
    with torch.no_grad():
        out = model(x.cuda(), meta.cuda())
    model.train(True)
    out_t = model(x.cuda(), meta.cuda())
    for task, _ in spec.heads:
        ref = z["logits_" + task]
        got = out[task].cpu().numpy()
        print(f"{name} {task}: max |logit err| {np.abs(got - ref).max():.3e} of {np.abs(ref).max():.3e}")
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-5, err_msg=task)
        assert (got.argmax(-1) == ref.argmax(-1)).all(), task
        assert torch.equal(out[task], out_t[task].detach()), task
    # and it is not the cos mode's answer
    cosm = build(spec, sd, "fp32", rotate=False)
    cosm.eval()
    with torch.no_grad():
        out_c = cosm(x.cuda(), meta.cuda())
    assert max((out_c[t] - out[t]).abs().max().item() for t in out) > 1e-3


@pytest.mark.parametrize("name", list(MODEL_HEADS))
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_matches_the_uncast_reference(name, dtype, golden_dir):
    """test_gpu_headdim.py's bounds where the fixture carries the figure: loss 2e-4 (fp32); per-tensor gradient norms 5e-3 and the
    recorded slices rtol 5e-3 / atol 5e-6 (fp32); attn.freqs in full at 2e-3 (fp32) / 0.10 (bf16) of its norm; the root of the summed
    squared norm errors 1e-3 (fp32) / 5e-2 (bf16).  The recompute plan's logits are the kept-activation plan's bit for bit, its gradients
    within that file's 1e-5 of each tensor's norm."""
    spec, z, sd, x, meta = load(name, golden_dir)
    model = build(spec, sd, dtype)
    model.train(True)
    out = model(x.cuda(), meta.cuda())
    loss = O.probe_loss(out)
    if dtype == "fp32":
        assert abs(loss.item() - float(z["loss"])) < 2e-4 * max(1.0, abs(float(z["loss"])))
    else:
        assert abs(loss.item() - float(z["loss"])) <= 3e-2 * max(1.0, abs(float(z["loss"])))
    loss.backward()
    names = [str(n) for n in z["grad_names"]]
    got = dict(model.named_parameters())
    assert sorted(got) == names
    num = den = 0.0
    for i, k in enumerate(names):
        ref_norm = float(z["grad_norms"][i])
        n = got[k].grad.double().norm().item()
        num += (n - ref_norm) ** 2
        den += ref_norm ** 2
        if dtype == "fp32":
            assert abs(n - ref_norm) <= 5e-3 * max(ref_norm, 1e-3), (k, n, ref_norm)
            np.testing.assert_allclose(got[k].grad.reshape(-1)[:8].float().cpu().numpy(), z["gradslice_" + k], rtol=5e-3, atol=5e-6, err_msg=k)
        if k.endswith("attn.freqs"):
            ref = torch.from_numpy(z["gradfull_" + k])
            err, denom = (got[k].grad.float().cpu() - ref).norm().item(), ref.norm().item()
            print(f"{name} {dtype} {k}: |err| {err:.3e} of {denom:.3e}")
            tol, floor = (2e-3, 1e-3) if dtype == "fp32" else (0.10, 1e-2)
            assert err <= tol * max(denom, floor), (k, err, denom)
    assert (num / den) ** 0.5 <= (1e-3 if dtype == "fp32" else 5e-2), (num / den) ** 0.5
    ga = grads_of(model)
    model.zero_grad(set_to_none=True)
    out_b = model(x.cuda(), meta.cuda(), force_checkpointing=True)
    for t in out:
        assert torch.equal(out[t], out_b[t]), t
    O.probe_loss(out_b).backward()
    gb = grads_of(model)
    for k in ga:  # (the order of the float atomics of several backward kernels varies from run to run: test_gpu_headdim.py's bound)
        e = (ga[k] - gb[k]).norm().item()
        assert e <= 1e-5 * ga[k].norm().item() + 1e-7, (k, e)


def test_fp8_plan_accepts_the_mode():
    """fp8 (MXFP8 qkv / fc1 / fc2 products, bf16 attention) with rotation, against the bf16 rotate plan: the forward bound
    test_fp8_mode_sm_b24_against_oracle_and_bf16 states for fp8 (0.12 x the logit scale), different logits (the fp8 kernels ran), and
    finite gradients from the kept and the recompute plan."""
    spec = O.Spec(heads=(("taxa_L10", 1000), ("taxa_L20", 300)))
    Bm = 8
    sd = O.seeded_state_dict(O.param_shapes(spec), 777)
    x, meta = O.seeded_inputs(spec, Bm, 224, 778)
    model = build(spec, sd, "bf16", img=224)
    model.train(True)
    out_bf = {t: v.detach().float().clone() for t, v in model(x.cuda(), meta.cuda()).items()}
    model.set_compute_dtype("fp8")
    assert model.compute_dtype == "fp8"
    for ck in (False, True):
        model.zero_grad(set_to_none=True)
        out = model(x.cuda(), meta.cuda(), force_checkpointing=ck)
        for t in out:
            scale = max(1.0, out_bf[t].abs().max().item())
            assert (out[t].float() - out_bf[t]).abs().max().item() <= 0.12 * scale, t
            assert not torch.equal(out[t].float(), out_bf[t]), t
        O.probe_loss(out).backward()
        assert all(torch.isfinite(p_.grad).all() for p_ in model.parameters())
    model.eval()
    with torch.no_grad():
        ev = model(x.cuda(), meta.cuda())
    for t in ev:
        assert (ev[t].float() - out_bf[t]).abs().max().item() <= 0.12 * max(1.0, out_bf[t].abs().max().item()), t


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_default_is_untouched(dtype, golden_dir):
    """no key == ROPE_ROTATE: false.  The two models hand lnx_plan_create the same bytes (the same native plan runs), their logits are
    equal bit for bit, and their gradients differ by no more than two runs of ONE model do: several weight-gradient kernels add floats
    atomically in an order that varies from run to run (stem.0.weight of one model differs from itself between two runs), so the bound
    is test_gpu_headdim.py's between two backward runs, 1e-5 of each tensor's norm."""
    spec, z, sd, x, meta = load("tiny_rot_hd64", golden_dir)
    res, cfgs = [], []
    for rotate in (None, False):
        model = build(spec, sd, dtype, rotate=rotate)
        cfgs.append(bytes(model._make_cfg(2, 64, 64, True)))
        model.train(True)
        out = model(x.cuda(), meta.cuda())
        O.probe_loss(out).backward()
        res.append(({t: v.detach().clone() for t, v in out.items()}, grads_of(model)))
    for t in res[0][0]:
        assert torch.equal(res[0][0][t], res[1][0][t]), t
    assert cfgs[0] == cfgs[1]
    exact = sum(int(torch.equal(res[0][1][k], res[1][1][k])) for k in res[0][1])
    print(f"{dtype}: {exact} of {len(res[0][1])} gradient tensors equal bit for bit")
    for k in res[0][1]:
        e = (res[0][1][k] - res[1][1][k]).norm().item()
        assert e <= 1e-5 * res[0][1][k].norm().item() + 1e-7, (k, e)
