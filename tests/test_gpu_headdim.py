"""Attention head_dim 32 and 128 on the GPU: the tiled kernels, the RoPE tables and the freqs-gradient folds against an fp64
restatement, and whole models against fixtures recorded from the reference (make_golden_headdim.py) and the oracle.
Tolerances are the head_dim-64 tests' at the same dtype (test_gpu_ops.test_attention_fwd_bwd / _probability_dropout,
test_gpu_model.test_forward_fp32_matches_reference / test_backward_matches_oracle / test_drop_rate_training_matches_reference /
test_sm_b24_production_dispatch_matches_oracle / test_sm_b256_batch_invariance / test_fp8_mode_sm_b24_against_oracle_and_bf16)."""
import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model, ops
from oracle import mformer_oracle as O
from tests.cases import CASES, SEED, make_config, model_state_dict_from_oracle, plan_dropout_buffers

pytestmark = pytest.mark.gpu
DT = {L.F32: torch.float32, L.BF16: torch.bfloat16}
HEADS = {"tiny_hd32": (4, 8), "tiny_hd128": (1, 2), "tiny_hd_drop": (4, 2)}


def g(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------------------------------------------
def attn_ref(qkv, freqs, B, N, E, heads, hd, H, W, drop=None):
    """fp64 restatement of RoPE2DAttention between the qkv and proj Linears (rope_2d_mhsa.py:422-505) at any head_dim: cos-only
    pair scaling of the image tokens' q and k, q * hd^-0.5, softmax, optional probability multiplier [B, h, N, N], P v."""
    t = qkv.reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = t[0], t[1], t[2]
    n = torch.arange(H * W, dtype=torch.float64)
    theta = (n % W)[:, None, None] * freqs[0][None] + torch.div(n, W, rounding_mode="floor")[:, None, None] * freqs[1][None]
    c = torch.cos(theta).permute(1, 0, 2).repeat_interleave(2, -1)  # [heads, HW, hd]
    q = torch.cat([q[:, :, :E], q[:, :, E:] * c], 2) * hd ** -0.5
    k = torch.cat([k[:, :, :E], k[:, :, E:] * c], 2)
    a = torch.softmax(q @ k.transpose(-2, -1), -1)
    if drop is not None:
        a = a * drop
    return (a @ v).transpose(1, 2).reshape(B * N, heads * hd)


# N = H W + E: <= 64, 64 < N <= 256 (bf16 N <= 128 and > 128 take the 4- and 8-wave tiled kernels), > 256; E = N (no image tokens)
SHAPES = [(2, 2, 3, 5, 3), (1, 3, 10, 10, 3), (2, 2, 14, 14, 3), (1, 2, 20, 20, 4), (2, 3, 0, 0, 40)]


@pytest.mark.parametrize("hd", [32, 128])
@pytest.mark.parametrize("B,heads,H,W,E", SHAPES)
@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
def test_attention_fwd_bwd(hd, B, heads, H, W, E, dtype):
    N = H * W + E
    C_ = heads * hd
    gen = g(B + heads * 5 + N + hd)
    qkv = torch.randn(B * N, 3 * C_, generator=gen).cuda().to(DT[dtype])
    freqs = O.seeded_fill("t.attn.freqs", (2, heads, hd // 2), 7).cuda()
    rope = H * W > 0
    cos = dsin = None
    if rope:
        dsin = torch.full((2, H * W, heads, hd // 2), float("nan"), device="cuda")
        cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
        assert cos.shape == (H * W, heads, hd // 2)
    o = torch.full((B * N, C_), float("nan"), device="cuda", dtype=DT[dtype])
    lse = torch.empty(B, heads, N, device="cuda")
    ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads)
    qr = qkv.double().cpu().requires_grad_(True)
    fr = freqs.double().cpu().requires_grad_(True)
    ref = attn_ref(qr, fr, B, N, E, heads, hd, H, W)
    tol = 3e-5 if dtype == L.F32 else 2e-2
    torch.testing.assert_close(o.double().cpu(), ref.detach(), rtol=tol, atol=tol)
    d_o = torch.randn(B * N, C_, generator=gen).cuda().to(DT[dtype])
    dqkv = torch.full((B * N, 3 * C_), float("nan"), device="cuda", dtype=DT[dtype])
    delta = torch.empty(B, heads, N, device="cuda")
    dfreqs = torch.ones(2, heads, hd // 2, device="cuda")  # accumulated into: starts at 1
    ops.attn_bwd(qkv, cos, o, lse, d_o, dqkv, delta, B, N, E, heads, dsin=dsin, dfreqs=dfreqs if rope else None)
    ref.backward(d_o.double().cpu())
    tolb = 1e-4 if dtype == L.F32 else 4e-2
    torch.testing.assert_close(dqkv.double().cpu(), qr.grad, rtol=tolb, atol=tolb)
    if rope:
        dfreqs -= 1.0
        scale = fr.grad.abs().max().item()
        torch.testing.assert_close(dfreqs.double().cpu(), fr.grad, rtol=tolb, atol=tolb * max(scale, 1.0))


@pytest.mark.parametrize("hd", [32, 128])
def test_rope_tables(hd):
    """cos table and d cos / d freqs at head_dim / 2 frequencies per head, alone and batched with head_dim 64 tables (one launch
    per head_dim): the batched tables equal the single ones bit for bit."""
    heads, H, W = 3, 7, 9
    freqs = O.seeded_fill(f"t.cos.{hd}", (2, heads, hd // 2), 5).cuda()
    dsin = torch.empty(2, H * W, heads, hd // 2, device="cuda")
    cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
    torch.testing.assert_close(cos.cpu(), O.rope_cos_table(freqs.cpu(), H, W), rtol=0, atol=2e-6)
    fd = freqs.double().cpu().requires_grad_(True)
    O.rope_cos_table(fd, H, W).sum().backward()
    torch.testing.assert_close(dsin.double().cpu().sum(1), fd.grad, rtol=1e-5, atol=1e-4)
    entries, want = [], []
    for i, d in enumerate([hd, 64, hd, 64, 32 if hd == 128 else 128]):
        f = O.seeded_fill(f"t.cos.batch.{i}", (2, heads, d // 2), 9 + i).cuda()
        out = torch.full((H * W, heads, d // 2), float("nan"), device="cuda")
        ds = torch.full((2, H * W, heads, d // 2), float("nan"), device="cuda")
        entries.append((f, H, W, out, ds))
        d1 = torch.empty_like(ds)
        want.append((ops.rope_cos_table(f, H, W, dsin=d1), d1))
    ops.rope_cos_tables(entries)
    torch.cuda.synchronize()
    for (_, _, _, out, ds), (c1, d1) in zip(entries, want):
        assert torch.equal(out, c1) and torch.equal(ds, d1)


@pytest.mark.parametrize("hd", [32, 128])
@pytest.mark.parametrize("B,heads,H,W,E", [(2, 2, 3, 5, 3), (1, 3, 14, 14, 3), (1, 2, 24, 24, 4)])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
def test_attention_probability_dropout(hd, B, heads, H, W, E, dtype):
    N = H * W + E
    Np = (N + 63) // 64 * 64
    C_ = heads * hd
    rate = 0.25
    gen = g(B + heads * 3 + N + hd)
    qkv = torch.randn(B * N, 3 * C_, generator=gen).cuda().to(DT[dtype])
    freqs = O.seeded_fill("t.attn.freqs", (2, heads, hd // 2), 7).cuda()
    dsin = torch.empty(2, H * W, heads, hd // 2, device="cuda")
    cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
    mask = (torch.rand(B, heads, N, Np, generator=gen) >= rate).to(torch.uint8).cuda()
    o = torch.empty(B * N, C_, device="cuda", dtype=DT[dtype])
    lse = torch.empty(B, heads, N, device="cuda")
    ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads, drop_mask=mask, drop_rate=rate)
    qr = qkv.double().cpu().requires_grad_(True)
    fr = freqs.double().cpu().requires_grad_(True)
    ref = attn_ref(qr, fr, B, N, E, heads, hd, H, W, mask[..., :N].double().cpu() / (1.0 - rate))
    tol = 3e-5 if dtype == L.F32 else 2e-2
    torch.testing.assert_close(o.double().cpu(), ref.detach(), rtol=tol, atol=tol)
    d_o = torch.randn(B * N, C_, generator=gen).cuda().to(DT[dtype])
    dqkv = torch.full((B * N, 3 * C_), float("nan"), device="cuda", dtype=DT[dtype])
    delta = torch.empty(B, heads, N, device="cuda")
    dfreqs = torch.zeros(2, heads, hd // 2, device="cuda")
    ops.attn_bwd(qkv, cos, o, lse, d_o, dqkv, delta, B, N, E, heads, dsin=dsin, dfreqs=dfreqs, drop_mask=mask, drop_rate=rate)
    ref.backward(d_o.double().cpu())
    tolb = 1e-4 if dtype == L.F32 else 4e-2
    torch.testing.assert_close(dqkv.double().cpu(), qr.grad, rtol=tolb, atol=tolb)
    scale = fr.grad.abs().max().item()
    torch.testing.assert_close(dfreqs.double().cpu(), fr.grad, rtol=tolb, atol=tolb * max(scale, 1.0))


def test_postponed_folds_of_mixed_head_dims():
    """defer_freqs + one flush over calls of head_dim 32, 64 and 128 (one fold launch per head_dim): each equals its own fold."""
    cases = [(2, 2, 3, 5, 3, L.BF16, 32), (1, 3, 14, 14, 3, L.BF16, 64), (1, 2, 24, 24, 4, L.BF16, 128), (1, 2, 7, 7, 4, L.F32, 128),
             (2, 4, 14, 14, 3, L.F32, 32)]
    runs = []
    for i, (B, heads, H, W, E, dtype, hd) in enumerate(cases):
        N, C_ = H * W + E, heads * hd
        gen = g(300 + i)
        qkv = torch.randn(B * N, 3 * C_, generator=gen).cuda().to(DT[dtype])
        freqs = O.seeded_fill(f"t.attn.defer.hd.{i}", (2, heads, hd // 2), 7 + i).cuda()
        dsin = torch.empty(2, H * W, heads, hd // 2, device="cuda")
        cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
        o = torch.empty(B * N, C_, device="cuda", dtype=DT[dtype])
        lse = torch.empty(B, heads, N, device="cuda")
        ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads)
        d_o = torch.randn(B * N, C_, generator=gen).cuda().to(DT[dtype])
        runs.append(dict(args=(qkv, cos, o, lse, d_o), shape=(B, N, E, heads, hd), dsin=dsin))
    for r in runs:
        B, N, E, heads, hd = r["shape"]
        r["want"] = torch.ones(2, heads, hd // 2, device="cuda")
        ops.attn_bwd(*r["args"], torch.empty_like(r["args"][0]), torch.empty(B, heads, N, device="cuda"), B, N, E, heads, dsin=r["dsin"], dfreqs=r["want"])
    keep = []
    for r in runs:
        B, N, E, heads, hd = r["shape"]
        r["got"] = torch.ones(2, heads, hd // 2, device="cuda")
        dq, dl = torch.empty_like(r["args"][0]), torch.empty(B, heads, N, device="cuda")
        keep.append((dq, dl, ops.attn_bwd(*r["args"], dq, dl, B, N, E, heads, dsin=r["dsin"], dfreqs=r["got"], defer_freqs=True)))
    torch.cuda.synchronize()
    assert all(bool((r["got"] == 1).all()) for r in runs)
    ops.attn_bwd_flush()
    torch.cuda.synchronize()
    for r in runs:
        assert not bool((r["got"] == 1).all())
        torch.testing.assert_close(r["got"], r["want"], rtol=1e-5, atol=1e-5 * float(r["want"].abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# model level against the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------------------
def spec_of(name):
    a = CASES["tiny_a"]
    return O.Spec(conv_dims=a.conv_dims, conv_depths=a.conv_depths, rope_depths=a.rope_depths, rope_heads=HEADS[name], heads=a.heads)


def load(name, golden_dir):
    spec = spec_of(name)
    z = np.load(f"{golden_dir}/{name}.npz", allow_pickle=False)
    sd = O.seeded_state_dict(O.param_shapes(spec), SEED)
    return spec, z, sd, torch.from_numpy(z["x"]), torch.from_numpy(z["meta"])


def build(spec, sd, dtype, img=64, **cfg_kw):
    cfg = make_config(spec, img)
    for k, v in cfg_kw.items():
        setattr(cfg.MODEL, k, v)
    model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype(dtype)
    return model


def grads_of(model):
    return {k: p_.grad.detach().clone() for k, p_ in model.named_parameters()}


@pytest.mark.parametrize("name", ["tiny_hd32", "tiny_hd128"])
def test_forward_fp32_matches_reference(name, golden_dir):
    spec, z, sd, x, meta = load(name, golden_dir)
    model = build(spec, sd, "fp32")
    model.eval()
    with torch.no_grad():
        out = model(x.cuda(), meta.cuda())
        feats = model._last_feats
    np.testing.assert_allclose(feats.cpu().numpy(), z["feats"], rtol=1e-4, atol=5e-5)
    for task, _ in spec.heads:
        ref = z["logits_" + task]
        got = out[task].cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=5e-5, err_msg=task)
        assert (got.argmax(-1) == ref.argmax(-1)).all(), task


@pytest.mark.parametrize("name", ["tiny_hd32", "tiny_hd128"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_matches_oracle_and_reference(name, dtype, golden_dir):
    """test_backward_matches_oracle's bounds; the recompute plan's gradients equal the kept-activation plan's."""
    spec, z, sd, x, meta = load(name, golden_dir)
    model = build(spec, sd, dtype)
    model.train(True)
    out = model(x.cuda(), meta.cuda())
    loss = O.probe_loss(out)
    if dtype == "fp32":
        assert abs(loss.item() - float(z["loss"])) < 2e-4 * max(1.0, abs(float(z["loss"])))
    loss.backward()
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    O.probe_loss(O.forward(osd, spec, x, meta, None)).backward()
    names = [str(n) for n in z["grad_names"]]
    got = dict(model.named_parameters())
    assert sorted(got) == names
    tot_err = tot_ref = 0.0
    bad = []
    for i, k in enumerate(names):
        gk = got[k].grad.float().cpu()
        ref = osd[k].grad
        denom, err = ref.norm().item(), (gk - ref).norm().item()
        tot_err += err * err
        tot_ref += denom * denom
        floor = 1e-3 * (1 if dtype == "fp32" else 10)
        if dtype == "fp32":
            assert abs(gk.double().norm().item() - z["grad_norms"][i]) <= 5e-3 * max(z["grad_norms"][i], 1e-3), k
        tol = 2e-3 if dtype == "fp32" else (0.25 if k.startswith("meta_") else 0.10)
        if err > tol * max(denom, floor):
            bad.append((k, err, denom))
    assert not bad, bad[:8]
    assert (tot_err / tot_ref) ** 0.5 <= (1e-3 if dtype == "fp32" else 5e-2)
    # recompute plan == kept activations
    ga = grads_of(model)
    model.zero_grad(set_to_none=True)
    out_b = model(x.cuda(), meta.cuda(), force_checkpointing=True)
    for t in out:
        assert torch.equal(out[t], out_b[t]), t
    O.probe_loss(out_b).backward()
    gb = grads_of(model)
    for k in ga:
        e = (ga[k] - gb[k]).norm().item()
        assert e <= 1e-5 * ga[k].norm().item() + 1e-7, (k, e)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_attention_dropout_matches_reference(dtype, golden_dir):
    """tiny_hd_drop: head_dim 32 on stage 3 and 128 on stage 4 in training with the reference's recorded keep masks
    (test_drop_rate_training_matches_reference's bounds), kept-activation and recompute plans."""
    spec, z, sd, x, meta = load("tiny_hd_drop", golden_dir)
    masks = []
    for i in range(int(z["n_masks"])):
        shape = tuple(int(v) for v in z[f"mask_shape_{i}"])
        n = int(np.prod(shape))
        masks.append(torch.from_numpy(np.unpackbits(z[f"mask_{i}"])[:n].reshape(shape).astype(np.bool_)))
    model = build(spec, sd, dtype, DROP_RATE=float(z["drop_rate"]), ATTN_DROP_RATE=float(z["attn_drop_rate"]))
    model._inject_dropout, model._inject_attn_dropout = plan_dropout_buffers(masks)
    names = [str(n) for n in z["grad_names"]]
    for ck in (False, True):
        model.zero_grad(set_to_none=True)
        model.train(True)
        out = model(x.cuda(), meta.cuda(), force_checkpointing=ck)
        for t, _ in spec.heads:
            ref = torch.from_numpy(z["logits_" + t])
            got = out[t].float().cpu()
            if dtype == "fp32":
                torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4 * max(1.0, ref.abs().max().item()), msg=t)
                assert (got.argmax(-1) == ref.argmax(-1)).all()
            else:
                assert (got - ref).abs().max().item() <= 0.05 * max(1.0, ref.abs().max().item()), t
        loss = O.probe_loss(out)
        assert abs(loss.item() - float(z["loss"])) <= (1e-4 if dtype == "fp32" else 3e-2) * max(1.0, abs(float(z["loss"])))
        loss.backward()
        got = dict(model.named_parameters())
        num = den = 0.0
        for i, k in enumerate(names):
            ref_norm = float(z["grad_norms"][i])
            n = got[k].grad.double().norm().item()
            num += (n - ref_norm) ** 2
            den += ref_norm ** 2
            if dtype == "fp32":
                assert abs(n - ref_norm) <= 1e-3 * max(ref_norm, 1e-3), (ck, k, n, ref_norm)
                np.testing.assert_allclose(got[k].grad.reshape(-1)[:8].float().cpu().numpy(), z["gradslice_" + k], rtol=5e-3, atol=5e-6, err_msg=k)
        assert (num / den) ** 0.5 <= (1e-3 if dtype == "fp32" else 5e-2), (ck, (num / den) ** 0.5)


# ---------------------------------------------------------------------------------------------------------------------------------
# production sizes: sm with NUM_HEADS [12, 24] (head_dim 32), xl with [8, 16] (head_dim 128)
# ---------------------------------------------------------------------------------------------------------------------------------
SM = O.Spec(rope_heads=(12, 24), heads=(("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20)), drop_path_rate=0.2)
XL = O.Spec(conv_dims=(256, 512, 1024, 2048), rope_depths=(22, 2), rope_heads=(8, 16),
            heads=(("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20)), drop_path_rate=0.2)


def _drop_scales(spec, B, seed):
    gen = g(seed)
    out = []
    for p_ in O.drop_call_probs(spec):
        out.append(None if p_ == 0.0 else torch.floor((1.0 - p_) + torch.rand(B, generator=gen)) / (1.0 - p_))
    return out


def _run(model, x, meta, drops):
    model.train(True)
    model._inject_drop = drops
    return model(x.cuda(), meta.cuda())


@pytest.mark.parametrize("which,B0,B", [("sm", 8, 256), ("xl", 4, 128)])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_production_shapes_against_oracle_and_batch_invariance(which, B0, B, dtype):
    """A small batch against the oracle (test_sm_b24_production_dispatch_matches_oracle's bounds), then the batch bench.py times
    with the small batch as its first rows: those rows' logits and (probe loss on them only) gradients equal the small batch's
    (test_sm_b256_batch_invariance's bounds).  bf16 runs the 8-wave tiled kernels at head_dim 128 and the 4-wave ones at 32."""
    spec = SM if which == "sm" else XL
    if which == "xl" and dtype == "fp32":
        B = 16  # the fp32 plan of xl at its bench batch does not fit beside the test process's other allocations
    sd = O.seeded_state_dict(O.param_shapes(spec), 777)
    x0, meta0 = O.seeded_inputs(spec, B0, 224, 778)
    drops0 = _drop_scales(spec, B0, 779)
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    oout = O.forward(osd, spec, x0, meta0, drops0)
    O.probe_loss(oout).backward()
    model = build(spec, sd, dtype, img=224)
    out0 = _run(model, x0, meta0, drops0)
    for t, _ in spec.heads:
        ref = oout[t].detach()
        got = out0[t].float().cpu()
        err = (got - ref).abs().max().item()
        scale = max(1.0, ref.abs().max().item())
        if dtype == "fp32":
            torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4 * scale, msg=t)
            assert (got.argmax(-1) == ref.argmax(-1)).all(), t
        else:
            assert err <= 0.025 * scale, (t, err, scale)
    O.probe_loss(out0).backward()
    tot_err = tot_ref = 0.0
    for k, p_ in model.named_parameters():
        tot_err += (p_.grad.float().cpu() - osd[k].grad).double().pow(2).sum().item()
        tot_ref += osd[k].grad.double().pow(2).sum().item()
    assert (tot_err / tot_ref) ** 0.5 <= (1e-3 if dtype == "fp32" else 5e-2)
    log0 = {t: v.detach().float().clone() for t, v in out0.items()}
    g0 = grads_of(model)
    model.zero_grad(set_to_none=True)
    del out0
    xf, metaf = O.seeded_inputs(spec, B - B0, 224, 780)
    dropsf = _drop_scales(spec, B - B0, 781)
    drops = [None if a is None else torch.cat([a, b]) for a, b in zip(drops0, dropsf)]
    out = _run(model, torch.cat([x0, xf]), torch.cat([meta0, metaf]), drops)
    O.probe_loss({t: v[:B0] for t, v in out.items()}).backward()
    for t, _ in spec.heads:
        scale = max(1.0, log0[t].abs().max().item())
        e = (out[t][:B0].detach().float() - log0[t]).abs().max().item() / scale
        assert e <= (1e-4 if dtype == "fp32" else 0.012), (t, e)
    e2 = r2 = 0.0
    for k, p_ in model.named_parameters():
        e2 += (p_.grad.double() - g0[k].double()).pow(2).sum().item()
        r2 += g0[k].double().pow(2).sum().item()
    assert (e2 / r2) ** 0.5 <= (2e-4 if dtype == "fp32" else 3e-2), (e2 / r2) ** 0.5


def test_fp8_forward_at_head_dim_128():
    """set_compute_dtype('fp8') (MXFP8 qkv / fc1 / fc2 products, bf16 attention) at head_dim 128: within the fp8 forward bound of
    test_fp8_mode_sm_b24_against_oracle_and_bf16 (0.12 x the logit scale)."""
    spec = O.Spec(rope_heads=(3, 6), heads=(("taxa_L10", 1000), ("taxa_L20", 300)))
    B = 8
    sd = O.seeded_state_dict(O.param_shapes(spec), 777)
    x, meta = O.seeded_inputs(spec, B, 224, 778)
    with torch.no_grad():
        oout = O.forward(sd, spec, x, meta, None)
    model = build(spec, sd, "fp8", img=224)
    assert model.compute_dtype == "fp8"
    model.eval()
    with torch.no_grad():
        out = model(x.cuda(), meta.cuda())
    for t, _ in spec.heads:
        ref = oout[t]
        got = out[t].float().cpu()
        scale = max(1.0, ref.abs().max().item())
        assert (got - ref).abs().max().item() <= 0.12 * scale, t
