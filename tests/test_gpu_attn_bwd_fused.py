"""The one-kernel resident attention backward (csrc/attention.hip attn_bwd_res_kernel, bf16 head_dim 64, N <= 224) against the dq /
dk-dv pair it replaces: the same inputs, LNX_ATTN_BWD_SPLIT (read per call) flipped between the two calls.

dqkv and delta are compared BIT FOR BIT, in the cos mode and in the rotating mode: both paths run the same loops and epilogues on
fragments that hold the same bits (the staged images hold what Chunk::value gave the pair).  dfreqs is a sum of LDS float adds whose
order is not fixed (freq_accum), so it is checked against fp64 within the bf16 tolerance of test_gpu_headdim.test_attention_fwd_bwd,
and dqkv is checked against the same fp64 restatement as well.

Sequence lengths: 1, 15, 16, 17 (one tile; a second wave's first row); 32, 33, 52 (a step of the 32-row image padding; the stage-4
length); 64, 65 (4 waves -> 16; wave 4's single row); 193, 199, 208, 209 (the 13th / 14th tile: waves beyond the sequence idle at both
barriers); 224 (the last one-kernel length); 225 and 256 (back on the pair).  There is no 8-wave instantiation, so 128 / 129 are no
boundary."""
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from oracle import mformer_oracle as O
from tests import rope_rotate_ref as RR
from tests.test_gpu_headdim import attn_ref

pytestmark = pytest.mark.gpu
B, HEADS, HD = 3, 2, 64
TOLB = 4e-2  # bf16 backward tolerance of test_gpu_headdim.test_attention_fwd_bwd
FUSED_NMAX = 224


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def grid_of(M):
    """(H, W) with H W = M image tokens, as square as M's divisors allow"""
    if M == 0:
        return 0, 0
    w = max(d for d in range(1, int(M ** 0.5) + 1) if M % d == 0)
    return M // w, w


_CACHE = {}


def case(N, E, mode):
    """inputs, the forward's outputs and the fp64 gradients of one (N, E, mode): computed once, shared, never modified"""
    key = (N, E, mode)
    if key in _CACHE:
        return _CACHE[key]
    H, W = grid_of(N - E)
    gen = torch.Generator().manual_seed(17 + 1000 * N + E)
    qkv = torch.randn(B * N, 3 * HEADS * HD, generator=gen).bfloat16()
    d_o = torch.randn(B * N, HEADS * HD, generator=gen).bfloat16()
    freqs = O.seeded_fill("t.attn.freqs", (2, HEADS, HD // 2), 7)
    c = dict(N=N, E=E, H=H, W=W, mode=mode, qkv=qkv.cuda(), d_o=d_o.cuda(), cos=None, sin=None, dsin=None)
    if H * W:
        if mode == "rotate":
            c["cos"], c["sin"] = ops.rope_cossin_table(freqs.cuda(), H, W)
        else:
            c["dsin"] = torch.empty(2, H * W, HEADS, HD // 2, device="cuda")
            c["cos"] = ops.rope_cos_table(freqs.cuda(), H, W, dsin=c["dsin"])
    c["o"] = torch.full((B * N, HEADS * HD), float("nan"), device="cuda", dtype=torch.bfloat16)
    c["lse"] = torch.full((B, HEADS, N), float("nan"), device="cuda")
    ops.attn_fwd(c["qkv"], c["cos"], c["o"], c["lse"], B, N, E, HEADS, **(dict(sin_tab=c["sin"]) if c["sin"] is not None else {}))
    if mode == "rotate":
        _, saved = RR.attn_fwd(qkv, freqs, B, N, E, HEADS, HD, H, W)
        c["ref_dqkv"], c["ref_dfreqs"] = RR.attn_bwd(d_o, saved, B, N, E, HEADS, HD, H, W)
    else:
        qr, fr = qkv.double().requires_grad_(True), freqs.double().requires_grad_(True)
        attn_ref(qr, fr, B, N, E, HEADS, HD, H, W).backward(d_o.double())
        c["ref_dqkv"], c["ref_dfreqs"] = qr.grad, fr.grad if H * W else None
    _CACHE[key] = c
    return c


def backward(c, monkeypatch, split, defer=False, dfreqs=None):
    """one lnx_attn_bwd of the case on the chosen path; returns dqkv, delta, dfreqs, the workspace and the launch count"""
    if split:
        monkeypatch.setenv("LNX_ATTN_BWD_SPLIT", "1")
    else:
        monkeypatch.delenv("LNX_ATTN_BWD_SPLIT", raising=False)
    N, E = c["N"], c["E"]
    dqkv = torch.full((B * N, 3 * HEADS * HD), float("nan"), device="cuda", dtype=torch.bfloat16)
    delta = torch.full((B, HEADS, N), float("nan"), device="cuda")
    rope = c["H"] * c["W"] > 0
    if dfreqs is None:
        dfreqs = torch.zeros(2, HEADS, HD // 2, device="cuda")
    kw = dict(sin_tab=c["sin"], grid_w=c["W"]) if c["sin"] is not None else {}
    ws = ops.attn_bwd(c["qkv"], c["cos"], c["o"], c["lse"], c["d_o"], dqkv, delta, B, N, E, HEADS, dsin=c["dsin"], dfreqs=dfreqs if rope else None,
                      defer_freqs=defer, **kw)
    launches = L.lib().lnx_last_attn_bwd_launches()
    if not defer:
        torch.cuda.synchronize()
    return dict(dqkv=dqkv, delta=delta, dfreqs=dfreqs, ws=ws, launches=launches)


def check(N, E, mode, monkeypatch):
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    c = case(N, E, mode)
    one = backward(c, monkeypatch, split=False)
    two = backward(c, monkeypatch, split=True)
    assert one["launches"] == (1 if N <= FUSED_NMAX else 2), (N, one["launches"])
    assert two["launches"] == 2
    assert L.lib().lnx_last_attn_kernel() == (L.ATTN_KERNEL_RES4 if N <= 64 else L.ATTN_KERNEL_RES8)
    ref = c["ref_dqkv"]
    err = float((one["dqkv"].double().cpu() - ref).abs().max())
    print(f"N={N} E={E} {mode}: launches {one['launches']}/{two['launches']}  max |dqkv - fp64| {err:.3e}")
    assert not bool(torch.isnan(one["dqkv"].float()).any()) and not bool(torch.isnan(one["delta"]).any())
    assert torch.equal(bits(one["dqkv"]), bits(two["dqkv"])), "dqkv differs from the pair's"
    assert torch.equal(bits(one["delta"]), bits(two["delta"])), "delta differs from the pair's"
    torch.testing.assert_close(one["dqkv"].double().cpu(), ref, rtol=TOLB, atol=TOLB)
    if c["ref_dfreqs"] is not None:
        scale = max(c["ref_dfreqs"].abs().max().item(), 1.0)
        for r in (one, two):
            torch.testing.assert_close(r["dfreqs"].double().cpu(), c["ref_dfreqs"], rtol=TOLB, atol=TOLB * scale)


LENGTHS = [1, 15, 16, 17, 32, 33, 52, 64, 65, 193, 199, 208, 209, 224, 225, 256]


@pytest.mark.parametrize("N", LENGTHS)
def test_one_kernel_equals_the_pair(N, monkeypatch):
    check(N, min(3, N - 1), "cos", monkeypatch)


@pytest.mark.parametrize("E", [0, "N"])  # E = 3 is in test_one_kernel_equals_the_pair
@pytest.mark.parametrize("N", [64, 199])
def test_extra_token_counts(N, E, monkeypatch):
    """no extra tokens (row 0 is an image token) and nothing but extra tokens (no tables, no freqs gradient)"""
    check(N, N if E == "N" else E, "cos", monkeypatch)


@pytest.mark.parametrize("N", [52, 199])
def test_rotating_mode(N, monkeypatch):
    """the ROT instantiations (4 and 16 waves): bit-equal to the pair's as well"""
    check(N, 3, "rotate", monkeypatch)


@pytest.mark.parametrize("N", [15, 16])
def test_deferred_fold_gives_the_bits_of_the_immediate_one(N, monkeypatch):
    """Two one-kernel calls with defer_freqs and one lnx_attn_bwd_flush against the same two calls folded singly.  N <= 16: one wave
    makes every LDS add of a workgroup, in program order, so the partials are the same bits in every run and the folds can be
    compared bit for bit (as in test_gpu_rope_rotate.test_deferred_fold_gives_the_bits_of_the_immediate_one)."""
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    cs = [case(N, 3, "cos"), case(N, 0, "cos")]
    single = [backward(c, monkeypatch, split=False, dfreqs=torch.ones(2, HEADS, HD // 2, device="cuda")) for c in cs]
    later = [backward(c, monkeypatch, split=False, defer=True, dfreqs=torch.ones(2, HEADS, HD // 2, device="cuda")) for c in cs]
    torch.cuda.synchronize()
    assert all(r["launches"] == 1 for r in single + later)
    assert all(bool((r["dfreqs"] == 1).all()) for r in later)  # nothing folded yet
    ops.attn_bwd_flush()
    torch.cuda.synchronize()
    for a, b_ in zip(single, later):
        assert not bool((a["dfreqs"] == 1).all())
        assert torch.equal(a["dfreqs"], b_["dfreqs"])
        assert torch.equal(bits(a["dqkv"]), bits(b_["dqkv"]))


def test_deferred_fold_on_a_multi_wave_shape(monkeypatch):
    """the bound test_gpu_headdim.test_postponed_folds_of_mixed_head_dims applies between a postponed and an immediate fold"""
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    cs = [case(199, 3, "cos"), case(52, 3, "cos")]
    single = [backward(c, monkeypatch, split=False, dfreqs=torch.ones(2, HEADS, HD // 2, device="cuda")) for c in cs]
    later = [backward(c, monkeypatch, split=False, defer=True, dfreqs=torch.ones(2, HEADS, HD // 2, device="cuda")) for c in cs]
    ops.attn_bwd_flush()
    torch.cuda.synchronize()
    for a, b_ in zip(single, later):
        torch.testing.assert_close(b_["dfreqs"], a["dfreqs"], rtol=1e-5, atol=1e-5 * float(a["dfreqs"].abs().max()))
