"""DropPath compaction: the device-built sample lists (lnx_drop_partition) and the kernels that work on compact rows -- the NT GEMM
families with `m_dev` / `perm` and the row copy that goes with their residual form (lnx_copy_dropped_rows), the weight-gradient GEMMs with
`m_dev`, lnx_scale_cast_compact, LayerNorm and attention with their lists, and the model with the switch on against off.

Compact rows of a call: row m' stands for sample perm[m' // rps], token m' % rps; rows >= m_eff = nkeep * rps are nobody's.  Every test
poisons those rows of the inputs with NaN and prefills the outputs with a sentinel: a kernel that reads or writes them shows."""
import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _i32(v):
    return torch.tensor([v], device="cuda", dtype=torch.int32)


def _partition_ref(sc):
    """numpy stable partition of the sample indices by `multiplier != 0`: perm, nkeep, inverse"""
    keep = np.flatnonzero(sc != 0.0)
    drop = np.flatnonzero(sc == 0.0)
    perm = np.concatenate([keep, drop]).astype(np.int32)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(perm.size, dtype=np.int32)
    return perm, int(keep.size), inv


PATTERNS = ["none_dropped", "all_dropped", "first_only", "last_only", "alternating", "random", "odd_values"]


def _pattern(name, B, rng):
    keep = 1.0 / 0.8
    sc = np.full(B, keep, dtype=np.float32)
    if name == "all_dropped":
        sc[:] = 0.0
    elif name == "first_only":
        sc[0] = 0.0
    elif name == "last_only":
        sc[-1] = 0.0
    elif name == "alternating":
        sc[::2] = 0.0
    elif name == "random":
        sc[rng.random(B) < 0.3] = 0.0
    elif name == "odd_values":  # multipliers other than 0 and 1 / keep: only an exact zero is a drop (-0.0 is one, a denormal is not)
        vals = np.array([0.0, -0.0, 1e-45, -3.5, 7.0, np.inf, keep, 0.0], dtype=np.float32)
        sc = vals[rng.integers(0, vals.size, B)]
    return sc


@pytest.mark.parametrize("B", [1, 7, 64, 300])
def test_partition_matches_numpy(B):
    rng = np.random.default_rng(B)
    scales = np.stack([_pattern(n, B, rng) for n in PATTERNS])
    rps = [1 + 3 * c for c in range(len(PATTERNS))]
    lists = ops.drop_partition(torch.from_numpy(scales).cuda(), rows_per_sample=rps)
    torch.cuda.synchronize()
    got = lists.lists.cpu().numpy()
    for c, name in enumerate(PATTERNS):
        perm, nkeep, inv = _partition_ref(scales[c])
        assert got[c, 0] == nkeep and got[c, 1] == nkeep * rps[c], (name, got[c, :2], nkeep)
        assert np.array_equal(got[c, 2:2 + B], perm), name
        assert np.array_equal(got[c, 2 + B:2 + 2 * B], inv), name


def test_partition_honours_the_call_mask():
    B = 9
    rng = np.random.default_rng(3)
    scales = np.stack([_pattern("random", B, rng) for _ in range(3)])
    lists = ops.drop_partition(torch.from_numpy(scales).cuda(), call_mask=[1, 0, 1])
    got = lists.lists.cpu().numpy()
    assert not got[1].any()  # (drop_partition hands out zeros: the masked call's list was not written)
    for c in (0, 2):
        perm, nkeep, inv = _partition_ref(scales[c])
        assert got[c, 0] == nkeep and got[c, 1] == nkeep and np.array_equal(got[c, 2:2 + B], perm) and np.array_equal(got[c, 2 + B:], inv)


# ---------------------------------------------------------------------------------------------------------------------------------
# NT GEMM, per family
# ---------------------------------------------------------------------------------------------------------------------------------
# family -> (environment that forces it, storage type, N, K): the hooks of test_nt_v7_forced_every_form / test_nt_v9_forced_every_form;
# the one-shot kernels are what is left when both persistent ones are switched off (256x256 where N % 256 == 0, else 256x128), the
# 128x128 kernel takes fp32 storage, and bf16 products of fewer than 1024 rows (nt_v2_ok)
FAMILIES = {
    "v1_f32": (dict(), L.F32, 384, 384, L.NT_KERNEL_V1),
    "v1_bf16": (dict(), L.BF16, 384, 384, L.NT_KERNEL_V1),
    "v2": (dict(LNX_NT_V7="0", LNX_NT_V9="0"), L.BF16, 384, 384, L.NT_KERNEL_V2),
    "v4": (dict(LNX_NT_V7="0", LNX_NT_V9="0"), L.BF16, 1536, 384, L.NT_KERNEL_V4),
    "v7": (dict(LNX_NT_V7="1"), L.BF16, 384, 384, L.NT_KERNEL_V7),
    "v7_deep": (dict(LNX_NT_V7="1"), L.BF16, 384, 1536, L.NT_KERNEL_V7),
    "v9": (dict(LNX_NT_V7="0", LNX_NT_V9="1"), L.BF16, 1536, 384, L.NT_KERNEL_V9),
}
FORMS = ["plain", "fc1d", "mul_aux", "res"]


def _nt_call(form, A, W, bias, aux, res, rowscale, rps, out, c2, **kw):
    if form == "plain":
        ops.gemm_nt(A, W, out, **kw)
    elif form == "fc1d":
        ops.gemm_nt(A, W, out, bias=bias, act=L.ACT_GELU_D, c2=c2, **kw)
    elif form == "mul_aux":
        ops.gemm_nt(A, W, out, act=L.ACT_MUL_AUX, aux=aux, **kw)
    else:
        ops.gemm_nt(A, W, out, bias=bias, res=res, rowscale=rowscale, rows_per_sample=rps, **kw)


def _kept_counts(B, rps, form):
    """(nkeep or None, m_eff): nothing, one sample, an effective M inside a tile, all; and -- where the form does not tie m_eff to whole
    samples -- an effective M on a 256-row tile edge"""
    out = [(0, 0), (1, rps), (B // 2 + 1, (B // 2 + 1) * rps), (B, B * rps)]
    if form != "res":
        out.append((None, 256 * max(1, (B * rps) // 512)))
    return out


def _nt_cases():
    """family x form x (rps, B).  gemm_nt_v7 does not carry the GELU' second output (nt_v7_ok), so that pair does not exist; the one-shot
    256x256 kernel is only chosen where it wins on whole rounds of tiles (big_tile_wins: 22 row tiles at N = 1536), hence its larger B;
    the 128x128 kernel takes a bf16 product of 256 < M < 1024 rows (at or below 256 the full-row reference call would go to the skinny kernel)."""
    shapes = {"v4": [(52, 108), (199, 28)], "v1_bf16": [(52, 12), (199, 4)]}
    for family in FAMILIES:
        for form in FORMS:
            if family.startswith("v7") and form == "fc1d":
                continue
            for rps, B in shapes.get(family, [(52, 24), (199, 12)]):
                yield family, form, rps, B


@pytest.mark.parametrize("family,form,rps,B", list(_nt_cases()))
def test_nt_compact_rows(family, form, rps, B, monkeypatch):
    env, dtype, N, K, kind = FAMILIES[family]
    for k in ("LNX_NT_V7", "LNX_NT_V9"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tdt = torch.float32 if dtype == L.F32 else torch.bfloat16
    M = B * rps
    g = torch.Generator().manual_seed(M + N + K)
    A0 = torch.randn(M, K, generator=g).cuda().to(tdt)
    W = (torch.randn(N, K, generator=g) * K**-0.5).cuda().to(tdt)
    bias = torch.randn(N, generator=g).cuda()
    aux0 = torch.randn(M, N, generator=g).cuda().to(tdt)
    res = torch.randn(M, N, generator=g).cuda()
    odt = torch.float32 if (form == "res" or dtype == L.F32) else tdt
    for nkeep, m_eff in _kept_counts(B, rps, form):
        # the list: a random set of nkeep kept samples (res form), multipliers 1 / keep and -- for one kept sample -- another value
        sc = np.zeros(B, dtype=np.float32)
        if nkeep is not None:
            sc[np.random.default_rng(nkeep).permutation(B)[:nkeep]] = 1.25
            if nkeep:
                sc[np.flatnonzero(sc)[0]] = -0.75
        perm_np, _, _ = _partition_ref(sc)
        rowscale = torch.from_numpy(sc).cuda()
        perm = torch.from_numpy(perm_np).cuda()
        # reference: the same call, same family, on the same compact rows without m_dev -- and for the residual form on res / rowscale
        # gathered into compact order, identity perm
        ref = torch.full((M, N), SENTINEL, device="cuda", dtype=odt)
        ref_c2 = torch.full((M, N), SENTINEL, device="cuda", dtype=tdt)
        res_c = res.view(B, rps, N)[perm.long()].reshape(M, N).contiguous()
        _nt_call(form, A0, W, bias, aux0, res_c, rowscale[perm.long()].contiguous(), rps, ref, ref_c2)
        assert L.lib().lnx_last_nt_kernel() == kind, (family, L.lib().lnx_last_nt_kernel())
        # the compact call: rows >= m_eff of the inputs poisoned, outputs prefilled
        A, aux = A0.clone(), aux0.clone()
        A[m_eff:] = float("nan")
        aux[m_eff:] = float("nan")
        out = torch.full((M, N), SENTINEL, device="cuda", dtype=odt)
        c2 = torch.full((M, N), SENTINEL, device="cuda", dtype=tdt)
        _nt_call(form, A, W, bias, aux, res, rowscale, rps, out, c2, m_dev=_i32(m_eff), perm=perm if form == "res" else None)
        assert L.lib().lnx_last_nt_kernel() == kind, (family, L.lib().lnx_last_nt_kernel())
        torch.cuda.synchronize()
        tag = f"{family} {form} rps={rps} m_eff={m_eff}"
        assert not torch.isnan(out).any() and not torch.isnan(c2).any(), tag
        if form == "res":
            out_c = out.view(B, rps, N)[perm.long()].reshape(M, N)  # compact order
            assert torch.equal(out_c[:m_eff], ref[:m_eff]), tag
            assert torch.equal(out_c[m_eff:], torch.full_like(out_c[m_eff:], SENTINEL)), tag  # rows of dropped samples: the product leaves them
            # ... to the row copy that goes with every such product (rope_block_fwd): C rows of dropped samples = res, bit for bit
            ops.copy_dropped_rows(res, out, perm=perm, nkeep=_i32(nkeep), rows_per_sample=rps)
            out_c = out.view(B, rps, N)[perm.long()].reshape(M, N)
            assert torch.equal(out_c[m_eff:], res_c[m_eff:]), tag
            assert torch.equal(out_c[:m_eff], ref[:m_eff]), tag  # kept rows: still the product's
        else:
            assert torch.equal(out[:m_eff], ref[:m_eff]), tag
            assert torch.equal(out[m_eff:], torch.full_like(out[m_eff:], SENTINEL)), tag
        if form == "fc1d":
            assert torch.equal(c2[:m_eff], ref_c2[:m_eff]) and torch.equal(c2[m_eff:], torch.full_like(c2[m_eff:], SENTINEL)), tag


@pytest.mark.parametrize("family", ["v1_f32", "v1_bf16", "v2", "v4", "v7", "v9"])
def test_nt_compact_residual_on_a_tile_edge(family, monkeypatch):
    """The residual form with an effective M on a 256-row tile edge: 64 rows per sample, 4 samples kept (of 88 where the one-shot 256x256
    kernel needs its 22 row tiles, of 12 where the 128x128 kernel takes bf16, else of 32)."""
    env, dtype, N, K, kind = FAMILIES[family]
    for k in ("LNX_NT_V7", "LNX_NT_V9"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tdt = torch.float32 if dtype == L.F32 else torch.bfloat16
    B, rps, nkeep = {"v4": 88, "v1_bf16": 12}.get(family, 32), 64, 4
    M = B * rps
    g = torch.Generator().manual_seed(5)
    A = torch.randn(M, K, generator=g).cuda().to(tdt)
    W = (torch.randn(N, K, generator=g) * K**-0.5).cuda().to(tdt)
    bias = torch.randn(N, generator=g).cuda()
    res = torch.randn(M, N, generator=g).cuda()
    sc = np.zeros(B, dtype=np.float32)
    sc[[3, 9, 10, B - 1]] = 1.25
    lists = ops.drop_partition(torch.from_numpy(sc[None]).cuda(), rows_per_sample=[rps])
    perm = lists.perm(0)
    res_c = res.view(B, rps, N)[perm.long()].reshape(M, N).contiguous()
    ref = torch.empty(M, N, device="cuda")
    ops.gemm_nt(A, W, ref, bias=bias, res=res_c, rowscale=torch.from_numpy(sc).cuda()[perm.long()].contiguous(), rows_per_sample=rps)
    assert L.lib().lnx_last_nt_kernel() == kind
    A[nkeep * rps:] = float("nan")
    out = torch.full((M, N), SENTINEL, device="cuda")
    ops.gemm_nt(A, W, out, bias=bias, res=res, rowscale=torch.from_numpy(sc).cuda(), rows_per_sample=rps, m_dev=lists.m_dev(0), perm=perm)
    assert L.lib().lnx_last_nt_kernel() == kind
    out_c = out.view(B, rps, N)[perm.long()].reshape(M, N)
    assert torch.equal(out_c[:nkeep * rps], ref[:nkeep * rps])
    assert torch.equal(out_c[nkeep * rps:], torch.full_like(out_c[nkeep * rps:], SENTINEL))
    ops.copy_dropped_rows(res, out, perm=perm, nkeep=lists.nkeep(0), rows_per_sample=rps)
    out_c = out.view(B, rps, N)[perm.long()].reshape(M, N)
    assert torch.equal(out_c[:nkeep * rps], ref[:nkeep * rps])            # kept rows: still the product's
    assert torch.equal(out_c[nkeep * rps:], res_c[nkeep * rps:])          # rows of dropped samples: res, bit for bit


@pytest.mark.parametrize("rps", [52, 199])
@pytest.mark.parametrize("Cc", [384, 768])
def test_copy_dropped_rows(Cc, rps):
    """lnx_copy_dropped_rows alone: every kept count from none (all rows copied) to all (nothing copied), the leading dimension the width
    or wider; rows of kept samples and the padding columns are not written."""
    B = 12
    M = B * rps
    g = torch.Generator().manual_seed(Cc + rps)
    for ld in (Cc, Cc + 8):
        src = torch.randn(M, ld, generator=g).cuda()
        for nkeep in (0, 1, 7, B - 1, B):
            sc = np.zeros(B, dtype=np.float32)
            sc[np.random.default_rng(nkeep).permutation(B)[:nkeep]] = 1.25
            lists = ops.drop_partition(torch.from_numpy(sc[None]).cuda(), rows_per_sample=[rps])
            dst = torch.full((M, ld), SENTINEL, device="cuda")
            ops.copy_dropped_rows(src, dst, perm=lists.perm(0), nkeep=lists.nkeep(0), rows_per_sample=rps, Cc=Cc, ld=ld)
            want = torch.full((B, rps, ld), SENTINEL, device="cuda")
            dropped = torch.from_numpy(np.flatnonzero(sc == 0.0)).cuda()
            want[dropped, :, :Cc] = src.view(B, rps, ld)[dropped, :, :Cc]
            assert torch.equal(dst.view(B, rps, ld), want), (ld, nkeep)


def test_nt_skinny_is_not_chosen_for_compact_rows():
    """The M <= 256 kernel does not carry m_dev: the dispatcher hands such a product to the 128x128 kernel."""
    A = torch.randn(208, 384, device="cuda").bfloat16()
    W = torch.randn(384, 384, device="cuda").bfloat16()
    out = torch.full((208, 384), SENTINEL, device="cuda", dtype=torch.bfloat16)
    ops.gemm_nt(A, W, out)
    assert L.lib().lnx_last_nt_kernel() == L.NT_KERNEL_SKINNY
    ref = out.clone()
    out.fill_(SENTINEL)
    ops.gemm_nt(A, W, out, m_dev=_i32(104))
    assert L.lib().lnx_last_nt_kernel() == L.NT_KERNEL_V1
    torch.testing.assert_close(out[:104].float(), ref[:104].float(), rtol=8e-3, atol=8e-3)  # (another kernel: another summation order)
    assert torch.equal(out[104:], torch.full_like(out[104:], SENTINEL))


# ---------------------------------------------------------------------------------------------------------------------------------
# TN GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
# (B, rps): M = B rps.  The LDS-DMA kernel takes bf16 with M % 64 == 0 and M >= 4096 (tn_v2_ok), everything else the 128x128 kernel
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("splits", [0, 24])
@pytest.mark.parametrize("dtype,B,rps", [(L.BF16, 64, 199), (L.BF16, 80, 52), (L.BF16, 12, 199), (L.F32, 24, 52)])
def test_tn_compact_rows(dtype, B, rps, splits, deterministic):
    """dW / db over the kept rows only, whatever the rows behind them hold; bounds of tests/test_gpu_gemm.py's test_tn.  splits = 24 is more
    than the non-empty ranges of the small kept counts (64-row contraction tiles): the surplus splits add zeros."""
    tdt = torch.float32 if dtype == L.F32 else torch.bfloat16
    M, N, K = B * rps, 384, 256
    g = torch.Generator().manual_seed(M + splits)
    dY0 = torch.randn(M, N, generator=g).cuda().to(tdt)
    A0 = torch.randn(M, K, generator=g).cuda().to(tdt)
    was = L.is_deterministic()
    L.lib().lnx_set_deterministic(int(deterministic))
    try:
        for m_eff in (0, rps, (B // 2 + 1) * rps, 256 * max(1, M // 512), M):
            dY, A = dY0.clone(), A0.clone()
            dY[m_eff:] = float("nan")
            A[m_eff:] = float("nan")
            for use_ws in (True, False):
                dW = torch.full((N, K), 0.5, device="cuda")
                db = torch.full((N,), 0.5, device="cuda")
                ws = torch.full((L.TN_WS_FLOATS,), float("nan"), device="cuda") if use_ws else None
                ops.gemm_tn(dY, A, dW, db=db, splits=splits, ws=ws, m_dev=_i32(m_eff))
                torch.cuda.synchronize()
                ref = dY0[:m_eff].double().T @ A0[:m_eff].double() + 0.5
                tag = f"M={M} m_eff={m_eff} ws={use_ws}"
                torch.testing.assert_close(dW.double(), ref, rtol=1e-4, atol=2e-5 * M**0.5, msg=lambda m: f"{tag}: {m}")
                torch.testing.assert_close(db.double(), dY0[:m_eff].double().sum(0) + 0.5, rtol=1e-4, atol=2e-5 * M**0.5, msg=lambda m: f"{tag} db: {m}")
                if use_ws and deterministic:
                    dW2 = torch.full((N, K), 0.5, device="cuda")
                    ops.gemm_tn(dY, A, dW2, splits=splits, ws=ws, m_dev=_i32(m_eff))
                    assert torch.equal(dW, dW2), tag
    finally:
        L.lib().lnx_set_deterministic(int(was))


# ---------------------------------------------------------------------------------------------------------------------------------
# lnx_scale_cast_compact
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,rps,Cc", [(12, 199, 384), (24, 52, 768)])
def test_scale_cast_compact(B, rps, Cc, out_dtype):
    rng = np.random.default_rng(B)
    sc = _pattern("random", B, rng)
    sc[np.flatnonzero(sc)[0]] = -0.75
    lists = ops.drop_partition(torch.from_numpy(sc[None]).cuda(), rows_per_sample=[rps])
    perm, nkeep, _ = _partition_ref(sc)
    M = B * rps
    x = torch.randn(M, Cc, device="cuda")
    out = torch.full((M, Cc), SENTINEL, device="cuda", dtype=out_dtype)
    ops.scale_cast_compact(x, out, M, Cc, perm=lists.perm(0), m_dev=lists.m_dev(0), rows_per_sample=rps, rowscale=torch.from_numpy(sc).cuda())
    want = (x.view(B, rps, Cc)[torch.from_numpy(perm).long().cuda()] * torch.from_numpy(sc[perm]).cuda().view(B, 1, 1)).reshape(M, Cc).to(out_dtype)
    assert torch.equal(out[:nkeep * rps], want[:nkeep * rps])
    assert torch.equal(out[nkeep * rps:], torch.full_like(out[nkeep * rps:], SENTINEL))


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward / backward with the sample gather (x side) and scatter (dx side)
# ---------------------------------------------------------------------------------------------------------------------------------
from tests import layernorm_ref as LR  # noqa: E402
from tests.test_gpu_layernorm import TOL as LN_TOL, within  # noqa: E402  (the LayerNorm tests' own bounds, for inputs at their scale)


def _ln_case(B, rps, Cc, seed):
    rng = np.random.default_rng(seed)
    sc1 = _pattern("random", B, rng)
    sc1[1] = 0.0          # at least one dropped under the first list ...
    sc1[0] = -0.75        # ... one kept with a multiplier of its own
    sc2 = _pattern("alternating", B, rng)
    sc2[1] = 1.25         # sample 1: dropped under list 1, kept under list 2
    lists = ops.drop_partition(torch.from_numpy(np.stack([sc1, sc2])).cuda(), rows_per_sample=[rps, rps])
    g = torch.Generator().manual_seed(seed)
    M = B * rps
    x = 2 * torch.randn(M, Cc, generator=g) + 0.5  # drawn as tests/test_gpu_layernorm.py draws them: its bounds are for this scale
    w = 1 + 0.2 * torch.randn(Cc, generator=g)
    b = 0.1 * torch.randn(Cc, generator=g)
    return sc1, sc2, lists, x, w, b


def _sample_rows(perm, n, rps):
    """rows of the first n samples of a list, in compact order"""
    return (torch.as_tensor(perm[:n], dtype=torch.int64)[:, None] * rps + torch.arange(rps)[None, :]).reshape(-1)


@pytest.mark.parametrize("ydt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,rps,Cc", [(12, 199, 384), (24, 52, 768)])
def test_layernorm_fwd_gather(B, rps, Cc, ydt):
    sc1, _, lists, x, w, b = _ln_case(B, rps, Cc, B + Cc)
    perm, nkeep, _ = _partition_ref(sc1)
    M, m_eff = B * rps, nkeep * rps
    y = torch.full((M, Cc), SENTINEL, device="cuda", dtype=ydt)
    mean = torch.full((M,), SENTINEL, device="cuda")
    rstd = torch.full((M,), SENTINEL, device="cuda")
    ops.layernorm_fwd(x.cuda(), w.cuda(), b.cuda(), y, 1e-5, mean=mean, rstd=rstd, perm=lists.perm(0), m_dev=lists.m_dev(0), rows_per_sample=rps)
    xs = x[_sample_rows(perm, nkeep, rps)]
    yr, mr, rr = LR.forward(xs, w, b, 1e-5, m_eff, Cc)
    within("y_f32" if ydt == torch.float32 else "y_bf16", y[:m_eff].cpu(), yr, what="gather")
    within("stat", rstd[:m_eff].cpu(), rr, what="gather rstd")
    err = (mean[:m_eff].double().cpu() - mr).abs() / (LN_TOL["stat"][0] * xs.double().abs().mean(-1))  # (relative to the row's mean |x|, as check_fwd)
    assert float(err.max()) <= 1.0, ("mean", float(err.max()))
    # bit-equal to the plain kernel on the gathered rows; rows behind the effective M untouched
    y2 = torch.empty(m_eff, Cc, device="cuda", dtype=ydt)
    ops.layernorm_fwd(xs.cuda(), w.cuda(), b.cuda(), y2, 1e-5)
    assert torch.equal(y[:m_eff], y2)
    assert torch.equal(y[m_eff:], torch.full_like(y[m_eff:], SENTINEL)) and torch.equal(mean[m_eff:], torch.full_like(mean[m_eff:], SENTINEL))


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,rps,Cc", [(12, 199, 384), (24, 52, 768)])
def test_layernorm_bwd_gather_scatter(B, rps, Cc, dt, defer):
    """dy / statistics compact under list 1, x / g by sample; dx2 compact under list 2 (another list); dw / db from kept rows only."""
    sc1, sc2, lists, x, w, _ = _ln_case(B, rps, Cc, B + Cc + 1)
    perm1, nk1, _ = _partition_ref(sc1)
    perm2, nk2, inv2 = _partition_ref(sc2)
    M, m_eff = B * rps, nk1 * rps
    gen = torch.Generator().manual_seed(B)
    rows1 = _sample_rows(perm1, nk1, rps)
    dy_c = torch.randn(M, Cc, generator=gen).to(dt)
    dy_c[m_eff:] = float("nan")
    g0 = torch.randn(M, Cc, generator=gen)
    mean_c = torch.full((M,), float("nan"))
    rstd_c = torch.full((M,), float("nan"))
    mean_c[:m_eff], rstd_c[:m_eff] = LR.stats_fp32(x[rows1], 1e-5, m_eff, Cc)
    g = g0.clone().cuda()
    dx2 = torch.full((M, Cc), SENTINEL, device="cuda", dtype=dt)
    dw = torch.zeros(Cc, device="cuda")
    db = torch.zeros(Cc, device="cuda")
    ws = torch.empty(2048 * 2 * Cc, device="cuda")
    ops.layernorm_bwd(dy_c.cuda(), x.cuda(), w.cuda(), mean_c.cuda(), rstd_c.cuda(), g, gin=g, dw=dw, db=db, ws=ws, defer=defer, dx2=dx2,
                      dx2_rowscale=torch.from_numpy(sc2).cuda(), dx2_rows_per_sample=rps, perm=lists.perm(0), m_dev=lists.m_dev(0), dx2_inv=lists.inv(1),
                      dx2_nkeep=lists.nkeep(1))
    if defer:
        ops.layernorm_bwd_flush()
    torch.cuda.synchronize()
    ref = LR.backward(dy_c[:m_eff], x[rows1], w, mean_c[:m_eff], rstd_c[:m_eff], m_eff, Cc, gin=g0[rows1])
    gc = g.cpu()
    assert not torch.isnan(gc).any() and not torch.isnan(dx2.float()).any() and not torch.isnan(dw).any()
    within("dx_f32", gc[rows1], ref["dx"], what="gather/scatter")  # (dx is fp32 whatever dy is stored as; the reference sees the rounded dy)
    dropped = _sample_rows(perm1[nk1:], B - nk1, rps)
    assert torch.equal(gc[dropped], g0[dropped])  # g rows of dropped samples: bit-unchanged
    # dx2: sample b at position inv2[b] of list 2, scaled by sc2[b], for the samples list 2 keeps -- those list 1 drops included
    gfin = gc.view(B, rps, Cc)
    want2 = (gfin[torch.as_tensor(perm2[:nk2], dtype=torch.int64)] * torch.from_numpy(sc2[perm2[:nk2]]).view(nk2, 1, 1)).reshape(nk2 * rps, Cc)
    if dt == torch.float32:
        assert torch.equal(dx2[:nk2 * rps].cpu(), want2)
    else:  # one rounding of that product to bf16
        within("dx_bf16", dx2[:nk2 * rps].cpu(), want2.double(), what="dx2")
    assert torch.equal(dx2[nk2 * rps:], torch.full_like(dx2[nk2 * rps:], SENTINEL))
    # column sums: tests/test_gpu_layernorm.py's bound, rel |ref| + abs . sum_m |term|
    for name, got in (("dw", dw), ("db", db)):
        within("cols", got.cpu(), ref[name], ref[name + "_abs"], what=name)


@pytest.mark.parametrize("with_dx2", [False, True])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,rps,Cc", [(12, 199, 384), (24, 52, 768), (12, 50, 192)])
def test_layernorm_bwd_compact_form_rounds_as_the_full_row_form(B, rps, Cc, dt, with_dx2):
    """Nothing dropped: the compact-row instantiation (identity perm) does the row arithmetic of the full-row one on the same rows, so dx
    and dx2 agree bit for bit -- per-row arithmetic does not depend on the form."""
    _, _, _, x, w, _ = _ln_case(B, rps, Cc, 3)
    M = B * rps
    sc = np.full(B, 1.25, dtype=np.float32)
    sc[0] = -0.75
    lists = ops.drop_partition(torch.from_numpy(sc[None]).cuda(), rows_per_sample=[rps])
    gen = torch.Generator().manual_seed(Cc)
    dy = torch.randn(M, Cc, generator=gen).to(dt).cuda()
    g0 = torch.randn(M, Cc, generator=gen).cuda()
    mean, rstd = LR.stats_fp32(x, 1e-5, M, Cc)
    got = []
    for compact in (False, True):
        g = g0.clone()
        dx2 = torch.full((M, Cc), SENTINEL, device="cuda", dtype=dt)
        kw = dict(dx2=dx2, dx2_rowscale=torch.from_numpy(sc).cuda()) if with_dx2 else {}
        if compact:
            kw.update(perm=lists.perm(0), m_dev=lists.m_dev(0))
            if with_dx2:
                kw.update(dx2_inv=lists.inv(0), dx2_nkeep=lists.nkeep(0))
        ops.layernorm_bwd(dy, x.cuda(), w.cuda(), mean.cuda(), rstd.cuda(), g, gin=g, dx2_rows_per_sample=rps, **kw)
        torch.cuda.synchronize()
        got.append((g, dx2))
    assert torch.equal(got[0][0], got[1][0])
    assert torch.equal(got[0][1], got[1][1])


# ---------------------------------------------------------------------------------------------------------------------------------
# attention forward / backward with nkeep
# ---------------------------------------------------------------------------------------------------------------------------------
def _grid_of(Mi):
    w = max(d for d in range(1, int(Mi ** 0.5) + 1) if Mi % d == 0)
    return Mi // w, w


ATTN_PATHS = {"bf16": (torch.bfloat16, {}), "bf16_pair": (torch.bfloat16, dict(LNX_ATTN_BWD_SPLIT="1")), "bf16_tiled": (torch.bfloat16, dict(LNX_ATTN_TILED="1")),
              "fp32": (torch.float32, {})}


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("mode", ["cos", "rotate"])
@pytest.mark.parametrize("N", [52, 199])
@pytest.mark.parametrize("path", list(ATTN_PATHS))
def test_attention_skips_dropped_samples(path, N, mode, defer, monkeypatch):
    dt, env = ATTN_PATHS[path]
    for k in ("LNX_ATTN_BWD_SPLIT", "LNX_ATTN_TILED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    from oracle import mformer_oracle as O
    B, heads, HD, E = 5, 2, 64, 1
    H, W = _grid_of(N - E)
    gen = torch.Generator().manual_seed(N)
    freqs = O.seeded_fill("t.attn.freqs", (2, heads, HD // 2), 7).cuda()
    sin = dsin = None
    if mode == "rotate":
        cos, sin = ops.rope_cossin_table(freqs, H, W)
    else:
        dsin = torch.empty(2, H * W, heads, HD // 2, device="cuda")
        cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
    kwf = dict(sin_tab=sin) if sin is not None else {}
    kwb = dict(sin_tab=sin, grid_w=W) if sin is not None else {}
    qkv0 = torch.randn(B * N, 3 * heads * HD, generator=gen).cuda().to(dt)
    do0 = torch.randn(B * N, heads * HD, generator=gen).cuda().to(dt)

    def run(nb, qkv, d_o, nkeep):
        o = torch.full((B * N, heads * HD), SENTINEL, device="cuda", dtype=dt)
        lse = torch.full((B, heads, N), SENTINEL, device="cuda")
        ops.attn_fwd(qkv, cos, o, lse, nb, N, E, heads, nkeep=nkeep, **kwf)
        dqkv = torch.full((B * N, 3 * heads * HD), SENTINEL, device="cuda", dtype=dt)
        delta = torch.full((B, heads, N), SENTINEL, device="cuda")
        dfreqs = torch.zeros(2, heads, HD // 2, device="cuda")
        ws = ops.attn_bwd(qkv, cos, o, lse, d_o, dqkv, delta, nb, N, E, heads, dsin=dsin, dfreqs=dfreqs, defer_freqs=defer, nkeep=nkeep, **kwb)
        if defer:
            ops.attn_bwd_flush()
        torch.cuda.synchronize()
        del ws
        return o, lse, dqkv, dfreqs

    for nk in (0, 3, B):
        qkv, d_o = qkv0.clone(), do0.clone()
        qkv[nk * N:] = float("nan")  # the dropped slots
        d_o[nk * N:] = float("nan")
        o, lse, dqkv, dfreqs = run(B, qkv, d_o, _i32(nk))
        for t in (o, lse, dqkv, dfreqs):
            assert not torch.isnan(t.float()).any(), (path, nk)
        assert torch.equal(o[nk * N:], torch.full_like(o[nk * N:], SENTINEL)) and torch.equal(dqkv[nk * N:], torch.full_like(dqkv[nk * N:], SENTINEL))
        assert torch.equal(lse[nk:], torch.full_like(lse[nk:], SENTINEL))
        if nk == 0:
            assert not dfreqs.any()
            continue
        o2, lse2, dqkv2, dfreqs2 = run(nk, qkv0, do0, None)  # the gathered batch: the kept samples alone
        assert torch.equal(o[:nk * N], o2[:nk * N]) and torch.equal(lse[:nk], lse2[:nk]) and torch.equal(dqkv[:nk * N], dqkv2[:nk * N]), (path, nk)
        tol = 4e-2 if dt == torch.bfloat16 else 1e-4  # the backward tolerances of tests/test_gpu_headdim.py's test_attention_fwd_bwd
        torch.testing.assert_close(dfreqs, dfreqs2, rtol=tol, atol=tol * max(float(dfreqs2.abs().max()), 1.0))


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: the switch on against the switch off
# ---------------------------------------------------------------------------------------------------------------------------------
from tests.test_gpu_model import _drop_scales, _grads, build, run as run_model  # noqa: E402
from tests.cases import load_case  # noqa: E402


def _injections(spec, B, drops):
    """the golden case's own multipliers, the seeded draw, and hand-made lists: one RoPE call fully kept, one fully dropped, one sample
    dropped in both branches of a block"""
    from oracle import mformer_oracle as O
    n = len(O.drop_call_probs(spec))
    n_conv = sum(spec.conv_depths)
    hand = [None] * n_conv
    for j in range(n - n_conv):
        v = torch.full((B,), 1.25)
        if j == 1:
            v[:] = 0.0           # one call fully dropped
        elif j in (2, 3):
            v[0] = 0.0           # block 1 of the first RoPE stage: sample 0 dropped in both branches
        elif j > 3:
            v[j % B] = 0.0
        hand.append(v)           # (j == 0: fully kept)
    return {"golden": drops, "seeded": _drop_scales(spec, B, 11), "hand": hand}


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny_b", "tiny_dp"])
def test_model_switch_on_equals_switch_off(name, dtype, ckpt, golden_dir):
    from oracle import mformer_oracle as O
    spec, z, sd, x, meta, drops = load_case(name, golden_dir)
    model = build(name, spec, sd, dtype)
    B = x.shape[0]
    xs, ms = x.cuda(), meta.cuda() if meta is not None else None
    try:
        for tag, inj in _injections(spec, B, drops).items():
            if inj is None or all(v is None for v in inj):
                continue
            res = {}
            for on in (False, True):
                model.set_drop_compact(on)
                model.zero_grad(set_to_none=True)
                model.train(True)
                model._inject_drop = inj
                before = model.drop_compact_branches()
                out = model(xs, ms, force_checkpointing=True) if ckpt else model(xs, ms)
                feats = model._last_feats.detach().clone()
                O.probe_loss(out).backward()
                ran = model.drop_compact_branches() - before
                assert (ran > 0) == on, (tag, on, ran)
                res[on] = ({k: v.detach().clone() for k, v in out.items()}, feats, _grads(model))
            for t in res[True][0]:
                assert torch.equal(res[True][0][t], res[False][0][t]), (tag, t)
            assert torch.equal(res[True][1], res[False][1]), tag
            # the gradients against the CPU oracle, inside test_backward_matches_oracle's bounds; the on / off difference is printed
            osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
            O.probe_loss(O.forward(osd, spec, x, meta, inj)).backward()
            worst_d = 0.0
            for k, p_ in model.named_parameters():
                parts = k.split(".")
                ck = f"head.{parts[3]}.fc.{parts[4]}" if (parts[0] == "head" and len(parts) >= 5 and parts[2] == "level_classifiers") else k
                ref = osd[ck].grad
                got = res[True][2][k].float().cpu()
                denom = max(ref.norm().item(), 1e-3 * (1 if dtype == "fp32" else 10))
                tol = 2e-3 if dtype == "fp32" else (0.25 if ck.startswith("meta_") else 0.10)
                assert (got - ref).norm().item() <= tol * denom, (tag, k, (got - ref).norm().item(), denom)
                worst_d = max(worst_d, (res[True][2][k].float() - res[False][2][k].float()).norm().item() / denom)
            print(f"[{name}/{dtype}/ckpt={ckpt}/{tag}] worst on/off gradient difference relative to the oracle's norm: {worst_d:.3e}")
    finally:
        model.set_drop_compact(None)


def test_gradnorm_forward_on_compact_rows(golden_dir):
    """One GradNorm forward + per-task backward_into after it: the lists of the one forward serve every backward."""
    spec, z, sd, x, meta, drops = load_case("tiny_dp", golden_dir)
    model = build("tiny_dp", spec, sd, "fp32")
    model.train(True)
    model._inject_drop = _injections(spec, x.shape[0], drops)["hand"]
    xs, ms = x.cuda(), meta.cuda() if meta is not None else None
    O_out = model(xs, ms)
    from oracle import mformer_oracle as O
    O.probe_loss(O_out).backward()  # binds the gradient arena
    T = len(spec.heads)

    def seeds(t, logits_t, dl_t):
        dl_t.copy_(torch.tanh(logits_t) * 0.01)

    res = {}
    try:
        for on in (False, True):
            model.set_drop_compact(on)
            before = model.drop_compact_branches()
            res[on] = model._task_backbone_grads(xs, ms, seeds, n_arenas=T).clone()
            assert (model.drop_compact_branches() > before) == on
    finally:
        model.set_drop_compact(None)
    for t in range(T):
        err = (res[True][t] - res[False][t]).norm().item()
        assert err <= 1e-5 * res[False][t].norm().item() + 1e-7, (t, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# the gate: where the old path is taken
# ---------------------------------------------------------------------------------------------------------------------------------
def test_gate_no_drop_pointer_keeps_the_old_path(golden_dir):
    from oracle import mformer_oracle as O
    spec, z, sd, x, meta, drops = load_case("tiny_dp", golden_dir)
    model = build("tiny_dp", spec, sd, "fp32")
    n = len(O.drop_call_probs(spec))
    before = model.drop_compact_branches()
    out = run_model(model, x, meta, [None] * n, train=True)
    O.probe_loss(out).backward()
    assert model.drop_compact_branches() == before
    # ... and an eval forward has no DropPath at all
    run_model(model, x, meta, None, train=False)
    assert model.drop_compact_branches() == before


def test_gate_drop_rate_keeps_the_old_path(golden_dir):
    """DROP_RATE > 0: the dropout masks are laid out by full rows, so every branch stays on full rows."""
    from linnaeus_amd import build_model
    from oracle import mformer_oracle as O
    from tests.cases import make_config, model_state_dict_from_oracle
    spec, z, sd, x, meta, drops = load_case("tiny_dp", golden_dir)
    cfg = make_config(spec, 64)
    cfg.MODEL.DROP_RATE = 0.2
    model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype("fp32")
    before = model.drop_compact_branches()
    out = run_model(model, x, meta, _injections(spec, x.shape[0], drops)["hand"], train=True)
    O.probe_loss(out).backward()
    assert model.drop_compact_branches() == before
    assert all(torch.isfinite(p_.grad).all() for p_ in model.parameters())


def test_gate_fp8_plan_keeps_the_old_path():
    """An fp8 plan's RoPE blocks run their products in MXFP8 (fp8_rows: M >= 256 rows, width >= 256): no compaction there; the same
    model in bf16 compacts."""
    from linnaeus_amd import build_model
    from oracle import mformer_oracle as O
    from tests.cases import make_config, model_state_dict_from_oracle
    spec = O.Spec(heads=(("taxa_L10", 10), ("taxa_L20", 5)), drop_path_rate=0.2)
    B = 8  # (stage 4 has 50 rows per sample: 400 rows, above the MXFP8 kernel's floor of 256 -- with fewer the stage runs, and compacts, in bf16)
    sd = O.seeded_state_dict(O.param_shapes(spec), 777)
    x, meta = O.seeded_inputs(spec, B, 224, 778)
    drops = _drop_scales(spec, B, 779)
    model = build_model(make_config(spec, 224), num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    for dtype, compacts in (("fp8", False), ("bf16", True)):
        model.set_compute_dtype(dtype)
        before = model.drop_compact_branches()
        out = run_model(model, x, meta, drops, train=True)
        O.probe_loss(out).backward()
        assert (model.drop_compact_branches() > before) == compacts, dtype
