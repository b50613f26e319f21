"""Deterministic mode (lnx_set_deterministic), op by op: every reduction that has a fixed-order route gives the same bits run to run,
adds its folded total to the destination exactly once, stays as accurate as the default route, and leaves the default route alone.

Inputs are randn * 2**randint(-12, 12): sums whose last bits depend on the order of the additions.  Every case runs at least 16
workgroups (or split-K slices) with at least two waves behind each output element, at a row count that is no multiple of the tile.

Tolerances: rtol and atol of the op's own test (tests/test_gpu_ops.py, tests/test_gpu_gemm.py), element by element.  Their atol was
set for sums of n terms of unit size; fp32 accumulation error grows with the size of the terms and with sqrt(n), so each element's
atol is multiplied by the root mean square of the terms summed into THAT element (computed in fp64 from the inputs, never below 1)
and, where this file sums more rows than the op's own test, by sqrt(rows here / rows there).  The attention case cannot split its
sum into per-element terms from outside the kernel and scales by the largest magnitude of the reference instead.

Calls that lack the scratch a fixed-order route needs refuse by name; that is asserted too.
"""
import ctypes as C

import pytest
import torch

import linnaeus_amd
from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from oracle import mformer_oracle as O

pytestmark = pytest.mark.gpu
DT = {L.F32: torch.float32, L.BF16: torch.bfloat16}
REPEATS = 8


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    linnaeus_amd.set_deterministic(False)


def wide(gen, *shape):
    """randn * 2**randint(-12, 12), element by element"""
    return torch.randn(*shape, generator=gen) * torch.pow(2.0, torch.randint(-12, 13, shape, generator=gen).float())


def gen_of(seed):
    return torch.Generator().manual_seed(seed)


def rms(terms, dims=0):
    """root mean square over the summed dimension(s) of the fp64 terms of a sum"""
    return terms.double().pow(2).mean(dims).sqrt()


def close(t, r, rt, at, scale):
    r = r.reshape(t.shape)
    bound = rt * r.abs() + at * (torch.as_tensor(scale, dtype=torch.float64).reshape(t.shape).clamp_min(1.0) if scale is not None else max(1.0, r.abs().max().item()))
    err = (t.double().cpu() - r).abs()
    assert bool((err <= bound).all()), f"worst element: error {err.max().item():.3e}, error / bound {(err / bound).max().item():.2f}"


def check_case(run, refs, rtol, atol, load=False, scales=None, grow=1.0):
    """run(init) -> list of reduced outputs; init(shape) fills a destination before the op accumulates into it.  refs: fp64 references;
    scales: per output, the rms of the terms of each element's sum; grow: sqrt(rows here / rows in the op's own test), at least 1."""
    zeros = lambda shape: torch.zeros(shape, device="cuda")  # noqa: E731
    scales = scales if scales is not None else [None] * len(refs)
    rtol = rtol if isinstance(rtol, list) else [rtol] * len(refs)  # (per output where the op's own test has one bound per output)
    atol = atol if isinstance(atol, list) else [atol] * len(refs)
    linnaeus_amd.set_deterministic(True)
    side = None
    if load:  # a long queue of small products on a second stream: workgroups of the op land wherever those leave room
        side = torch.cuda.Stream()
        a = torch.randn(256, 256, device="cuda")
        with torch.cuda.stream(side):
            for _ in range(400):
                a = torch.mm(a, a) * 1e-3
    outs = [run(zeros) for _ in range(REPEATS)]
    torch.cuda.synchronize()
    for o in outs[1:]:
        for t, t0 in zip(o, outs[0]):
            assert torch.equal(t, t0), "deterministic mode: two runs from the same inputs differ"
    # accumulation: the partial sums are folded first and added once, so p + g is exact
    pre = {}

    def prefilled(shape):
        pre[len(pre)] = torch.randn(shape, generator=gen_of(11 + len(pre))).cuda()
        return pre[len(pre) - 1].clone()

    acc = run(prefilled)
    torch.cuda.synchronize()
    for i, (t, g0) in enumerate(zip(acc, outs[0])):
        assert torch.equal(t, pre[i] + g0), "deterministic mode: destination += total is not one addition of the folded total"
    for t, r, rt, at, sc in zip(outs[0], refs, rtol, atol, scales):
        close(t, r, rt, at * max(1.0, grow), sc)
    # the default route still runs and is as accurate
    linnaeus_amd.set_deterministic(False)
    for t, r, rt, at, sc in zip(run(zeros), refs, rtol, atol, scales):
        close(t, r, rt, at * max(1.0, grow), sc)


# ------------------------------------------------------------------------------------------------ split-K weight gradients
@pytest.mark.parametrize("load", [False, True])
@pytest.mark.parametrize("M,dtype,ws", [(4096 + 40, L.BF16, False), (4096 + 40, L.F32, False), (4096 + 40, L.BF16, True), (8192, L.BF16, True),
                                        (8192, L.BF16, False)])
def test_tn(M, dtype, ws, load):
    """N x K = 96 x 64 fills 9 % of a 256 x 128 tile: the default route sums such sparse tiles by atomics whatever workspace it is given.
    M = 4136 runs the v1 kernel (no multiple of 64 rows), M = 8192 the v2 kernel with and without a workspace."""
    N, K = 96, 64
    gen = gen_of(M + dtype)
    dY = wide(gen, M, N).cuda().to(DT[dtype])
    A = wide(gen, M, K).cuda().to(DT[dtype])
    wsb = torch.empty(L.TN_WS_FLOATS, device="cuda") if ws else None
    refs = [dY.double().cpu().T @ A.double().cpu(), dY.double().cpu().sum(0)]

    def run(init):
        dW, db = init((N, K)), init((N,))
        ops.gemm_tn(dY, A, dW, db=db, ws=wsb)
        return [dW, db]

    y2, a2 = dY.double().cpu().pow(2), A.double().cpu().pow(2)
    check_case(run, refs, 1e-4, 2e-5 * M**0.5, load, scales=[(y2.T @ a2 / M).sqrt(), rms(dY.cpu())])


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("C_", [96, 384])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
def test_layernorm_bwd(C_, dtype):
    M = 2000
    gen = gen_of(C_ + dtype)
    x = (torch.randn(M, C_, generator=gen) * 2 + 0.5).cuda().to(DT[dtype])
    w = (1 + 0.2 * torch.randn(C_, generator=gen)).cuda()
    b = (0.1 * torch.randn(C_, generator=gen)).cuda()
    y = torch.empty(M, C_, device="cuda", dtype=DT[dtype])
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    ops.layernorm_fwd(x, w, b, y, 1e-6, mean=mean, rstd=rstd)
    dy = wide(gen, M, C_).cuda().to(DT[dtype])
    ws = torch.empty(2048 * 2 * C_, device="cuda")
    xr, wr, br = x.double().cpu(), w.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    O.layer_norm_last(xr, wr, br, 1e-6).backward(dy.double().cpu())

    def run(init):
        dx = torch.empty(M, C_, device="cuda")
        dw, db = init((C_,)), init((C_,))
        ops.layernorm_bwd(dy, x, w, mean, rstd, dx, dw=dw, db=db, ws=ws)
        return [dw, db]

    assert ops.layernorm_bwd_query(dy, x, w, mean, rstd, torch.empty(M, C_, device="cuda"), dw=w, db=b, ws=ws).grid >= 16
    xh = (xr - xr.mean(1, keepdim=True)) / torch.sqrt(xr.var(1, unbiased=False, keepdim=True) + 1e-6)
    check_case(run, [wr.grad, br.grad], 1e-4, 2e-4, scales=[rms(dy.double().cpu() * xh), rms(dy.cpu())], grow=(M / 77) ** 0.5)
    # without the workspace the column sums are float atomics: refused by name in the mode
    linnaeus_amd.set_deterministic(True)
    with pytest.raises(L.LnxError, match="lnx_layernorm_bwd: deterministic mode"):
        ops.layernorm_bwd(dy, x, w, mean, rstd, torch.empty(M, C_, device="cuda"), dw=torch.zeros(C_, device="cuda"), db=torch.zeros(C_, device="cuda"))


# ------------------------------------------------------------------------------------------------ depthwise 7x7 weight gradient
@pytest.mark.parametrize("load", [False, True])
@pytest.mark.parametrize("C_", [32, 96])
@pytest.mark.parametrize("xd,dyd", [(L.F32, L.F32), (L.F32, L.BF16), (L.BF16, L.F32), (L.BF16, L.BF16)])
def test_dwconv_wgrad(C_, xd, dyd, load):
    """fp32 operands: the VALU kernel; a bf16 operand: the MFMA kernel, in each of its compiled dtype pairs"""
    B, H, W = 2, 28, 28
    gen = gen_of(C_ + 2 * xd + dyd)
    x = wide(gen, B, H, W, C_).cuda().to(DT[xd])
    dy = wide(gen, B, H, W, C_).cuda().to(DT[dyd])
    # the MFMA kernel (any bf16 operand) rounds both operands of the products to bf16 and sums dy for the bias as given: the fp64
    # reference runs on what the kernel multiplies (tests/test_gpu_ops.py::test_dwconv_mfma)
    mfma = L.BF16 in (xd, dyd)
    r16 = (lambda t: t.bfloat16()) if mfma else (lambda t: t)
    xr = r16(x).double().cpu().permute(0, 3, 1, 2)
    wr = torch.zeros(C_, 1, 7, 7, dtype=torch.float64, requires_grad=True)
    O.depthwise_conv7(xr, wr, None).backward(r16(dy).double().cpu().permute(0, 3, 1, 2))
    gb = dy.double().cpu().sum((0, 1, 2))
    # (2 x 28 x 28 is four 14 x 28 tiles of the MFMA kernel, 32 of the VALU kernel's: 4 or more walkers behind every tap, C / 16 or
    # C / 32 channel blocks each)
    assert ops.dwconv7_wgrad_ws_floats(B, H, W, C_, xd, dyd) >= 4 * 50 * C_

    def run(init):
        dw, db = init((C_, 1, 7, 7)), init((C_,))
        ops.dwconv7_wgrad(x, dy, dw, db)
        return [dw, db]

    w2 = torch.zeros(C_, 1, 7, 7, dtype=torch.float64, requires_grad=True)  # sums of the squared terms: the same correlation on squares
    O.depthwise_conv7(xr.pow(2), w2, None).backward(r16(dy).double().cpu().permute(0, 3, 1, 2).pow(2))
    check_case(run, [wr.grad, gb], 1e-4, 2e-5 * (B * H * W) ** 0.5, load, scales=[(w2.grad / (B * H * W)).sqrt(), rms(dy.cpu(), (0, 1, 2))])


def test_dwconv_wgrad_refuses_missing_scratch():
    linnaeus_amd.set_deterministic(True)
    x = torch.randn(1, 8, 8, 32, device="cuda")
    a = L.DwconvWgradArgs()
    a.B, a.H, a.W, a.C = 1, 8, 8, 32
    dw, db = torch.zeros(32, 1, 7, 7, device="cuda"), torch.zeros(32, device="cuda")
    a.x, a.x_dtype, a.dy, a.dy_dtype, a.dw, a.db = x.data_ptr(), L.F32, x.data_ptr(), L.F32, dw.data_ptr(), db.data_ptr()
    assert L.lib().lnx_dwconv7_wgrad(C.byref(a), None) != 0 and b"lnx_dwconv7_wgrad: deterministic mode needs ws" in L.lib().lnx_last_error()
    torch.cuda.synchronize()
    assert dw.abs().sum().item() == 0


# ------------------------------------------------------------------------------------------------ element-wise reductions
@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
def test_layerscale_bwd(dtype):
    M, C_ = 3001, 96  # 10 rows a workgroup pass, 8 passes: 38 workgroups of 4 waves
    gen = gen_of(5 + dtype)
    gg = wide(gen, M, C_).cuda()
    z = wide(gen, M, C_).cuda().to(DT[dtype])
    gam = torch.randn(C_, generator=gen).cuda()
    ref = (gg.double().cpu() * z.double().cpu()).sum(0)

    def run(init):
        dz = torch.empty(M, C_, device="cuda", dtype=DT[dtype])
        dgam = init((C_,))
        ops.layerscale_bwd(gg, z, gam, None, 0, dz, dgam, M, C_)
        return [dgam]

    check_case(run, [ref], 1e-4, 1e-4, scales=[rms(gg.double().cpu() * z.double().cpu())], grow=(M / 150) ** 0.5)
    linnaeus_amd.set_deterministic(True)  # the entry point without scratch refuses by name
    dz, dgam = torch.empty(M, C_, device="cuda", dtype=DT[dtype]), torch.zeros(C_, device="cuda")
    rc = L.lib().lnx_layerscale_bwd(ops._p(gg), ops._p(z), dtype, ops._p(gam), None, 0, ops._p(dz), ops._p(dgam), M, C_, None)
    assert rc != 0 and b"lnx_layerscale_bwd: deterministic mode needs lnx_layerscale_bwd_ws" in L.lib().lnx_last_error()


def test_colsum_rows():
    M, C_ = 2000 + 7, 96  # 63 strips of 32 rows in the default route
    src = wide(gen_of(6), M, C_).cuda()

    def run(init):
        acc = init((C_,))
        ops.colsum_rows(src, C_, (0, 0, 0), acc, M, C_)
        return [acc]

    check_case(run, [src.double().cpu().sum(0)], 1e-5, 1e-5, scales=[rms(src.cpu())], grow=(M / 3) ** 0.5)


def test_agg2_bwd():
    M, C_ = 301, 96  # 29 workgroups in the default route
    gen = gen_of(7)
    a, b, dout = wide(gen, M, C_).cuda(), wide(gen, M, C_).cuda(), wide(gen, M, C_).cuda()
    w2 = torch.tensor([0.7, -0.3]).cuda()
    ad, bd, dd = a.double().cpu(), b.double().cpu(), dout.double().cpu()

    def run(init):
        da, dbb = torch.empty_like(a), torch.empty_like(b)
        dw2, db1 = init((2,)), init((1,))
        ops.agg2_bwd(dout, a, b, w2, da, dbb, dw2, db1, M, C_)
        return [dw2, db1]

    check_case(run, [torch.stack([(dd * ad).sum(), (dd * bd).sum()]), dd.sum().reshape(1)], 1e-5, 1e-5,
               scales=[torch.stack([rms(dd * ad, (0, 1)), rms(dd * bd, (0, 1))]), rms(dd, (0, 1)).reshape(1)], grow=(M * C_ / 320) ** 0.5)


# ------------------------------------------------------------------------------------------------ soft-label cross entropy
def test_softce_loss_sum():
    """loss_sum of two argument sets in one launch (the multi-task criterion's launch), 300 rows each"""
    from linnaeus_amd import loss as LS

    B, Cn = 300, 37
    gen = gen_of(8)
    xs = [(torch.randn(B, Cn, generator=gen) * 3).cuda() for _ in range(2)]
    ts = [torch.randint(0, Cn, (B,), generator=gen).cuda() for _ in range(2)]
    scale = [wide(gen, B).abs().cuda() for _ in range(2)]  # per-row multipliers of very different sizes
    refs = [(torch.nn.functional.cross_entropy(x.double().cpu(), t.cpu(), reduction="none") * s.double().cpu()).sum() * 0.5
            for x, t, s in zip(xs, ts, scale)]

    def run(init):
        totals = [init(()), init(())]
        rows = [torch.empty(B, device="cuda") for _ in range(2)]
        LS._launch_multi([(x, t, None, 0.0, None, None, s, 0.5, None, tot, None, 0, None, r) for x, t, s, r, tot in zip(xs, ts, scale, rows, totals)])
        return totals

    terms = [torch.nn.functional.cross_entropy(x.double().cpu(), t.cpu(), reduction="none") * sc.double().cpu() * 0.5 for x, t, sc in zip(xs, ts, scale)]
    check_case(run, refs, 1e-5, 1e-5, scales=[rms(t) for t in terms])
    linnaeus_amd.set_deterministic(True)  # no per-row buffer: refused by name
    with pytest.raises(L.LnxError, match="deterministic mode needs sum_ws"):
        LS._launch_multi([(xs[0], ts[0], None, 0.0, None, None, None, 1.0, None, torch.zeros((), device="cuda"), None)])


# ------------------------------------------------------------------------------------------------ attention backward (freqs gradient)
@pytest.mark.parametrize("HW,E", [((8, 8), 1), ((16, 16), 4)])  # N = 65: the resident kernels, N = 260: the tiled ones
@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
def test_attention_bwd_freqs(HW, E, dtype):
    B, heads, (H, W) = 2, 2, HW
    N, C_ = H * W + E, heads * 64
    gen = gen_of(N + dtype)
    qkv = torch.randn(B * N, 3 * C_, generator=gen).cuda().to(DT[dtype])
    freqs = O.seeded_fill("t.attn.freqs", (2, heads, 32), 7).cuda()
    dsin = torch.empty(2, H * W, heads, 32, device="cuda")
    cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
    o = torch.empty(B * N, C_, device="cuda", dtype=DT[dtype])
    lse = torch.empty(B, heads, N, device="cuda")
    ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads)
    # the gradient is linear in d_o: rows of very different sizes (a power of two per row keeps bf16 rows exact multiples)
    d_o = (torch.randn(B * N, C_, generator=gen) * torch.pow(2.0, torch.randint(-12, 13, (B * N, 1), generator=gen).float())).cuda().to(DT[dtype])
    qr, fr = qkv.double().cpu(), freqs.double().cpu().requires_grad_(True)
    t = qr.reshape(B, N, 3, heads, 64).permute(2, 0, 3, 1, 4)
    cr = O.rope_cos_table(fr, H, W)
    q = torch.cat([t[0][:, :, :E], O.rope_scale_pairs(t[0][:, :, E:], cr)], 2) * 0.125
    k = torch.cat([t[1][:, :, :E], O.rope_scale_pairs(t[1][:, :, E:], cr)], 2)
    ((torch.softmax(q @ k.transpose(-2, -1), -1) @ t[2]).transpose(1, 2).reshape(B * N, C_)).backward(d_o.double().cpu())

    def run(init):
        dqkv = torch.empty(B * N, 3 * C_, device="cuda", dtype=DT[dtype])
        delta = torch.empty(B, heads, N, device="cuda")
        dfreqs = init((2, heads, 32))
        ops.attn_bwd(qkv, cos, o, lse, d_o, dqkv, delta, B, N, E, heads, dsin=dsin, dfreqs=dfreqs)
        return [dfreqs]

    tolb = 1e-4 if dtype == L.F32 else 4e-2
    check_case(run, [fr.grad], tolb, tolb)


# ------------------------------------------------------------------------------------------------ conv-MLP backward
@pytest.mark.parametrize("load", [False, True])
@pytest.mark.parametrize("C_", [32, 96, 192])
def test_convmlp_bwd(C_, load):
    """The form with z (dgamma) and y (the block LayerNorm inside): C = 32 and 96 run the resident-weight kernel (12 and 24 workgroups of
    8 waves, several tiles a wave), C = 192 the streamed-weight kernel (24 workgroups, one 16-row tile a wave).  In the mode every wave
    leaves its column sums in a row of its own and the second stages fold the rows in order.  References as tests/test_gpu_ops.py:
    dgamma against fp64 on the stored z, the LayerNorm gradients against fp64 on the dln the kernel without the LayerNorm stores."""
    M, rps, bf = 3001, 50, torch.bfloat16
    gen = gen_of(C_)
    nb = (M + rps - 1) // rps
    y = (1.5 * torch.randn(M, C_, generator=gen) + 0.3).cuda().to(bf)
    lw, lb = (1.0 + 0.2 * torch.randn(C_, generator=gen)).cuda(), (0.1 * torch.randn(C_, generator=gen)).cuda()
    w1 = (torch.randn(4 * C_, C_, generator=gen) / C_**0.5).cuda().to(bf)
    b1 = (0.2 * torch.randn(4 * C_, generator=gen)).cuda()
    w2 = (torch.randn(C_, 4 * C_, generator=gen) / (4 * C_) ** 0.5).cuda().to(bf)
    b2 = (0.2 * torch.randn(C_, generator=gen)).cuda()
    gam = (0.5 + 0.3 * torch.randn(C_, generator=gen)).cuda()
    rs = (torch.rand(nb, generator=gen) > 0.3).float().cuda() * 1.25
    x = torch.randn(M, C_, generator=gen).cuda()
    ln = torch.empty(M, C_, device="cuda", dtype=bf)
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    out, z = torch.empty(M, C_, device="cuda"), torch.empty(M, C_, device="cuda", dtype=bf)
    ops.convmlp_fwd(None, w1, b1, w2, b2, gam, x, out, rowscale=rs, rows_per_sample=rps, z=z, y=y, ln_w=lw, ln_b=lb, ln_eps=1e-6, ln_out=ln, mean=mean, rstd=rstd)
    gout = wide(gen, M, C_).cuda()
    w2t, w1t = w2.t().contiguous(), w1.t().contiguous()
    e = lambda *sh: torch.empty(*sh, device="cuda", dtype=bf)  # noqa: E731
    dln0 = e(M, C_)  # the kernel without the LayerNorm and without z: no reduction in it, either mode
    ops.convmlp_bwd(gout, ln, None, w1, b1, w2t, w1t, gam, None, None, e(M, C_), dln0, None, rowscale=rs, rows_per_sample=rps)
    sd = rs.double().cpu().repeat_interleave(rps)[:M, None]
    yd = y.double().cpu()
    xh = (yd - yd.mean(1, keepdim=True)) / torch.sqrt(yd.var(1, unbiased=False, keepdim=True) + 1e-6)
    dl = dln0.double().cpu()
    refs = [(sd * gout.double().cpu() * z.double().cpu()).sum(0), (dl * xh).sum(0), dl.sum(0)]
    linnaeus_amd.set_deterministic(True)
    need = int(L.lib().lnx_convmlp_bwd_ws_floats(C_, M))
    linnaeus_amd.set_deterministic(False)
    assert need >= {32: 12, 96: 24, 192: 24}[C_] * 4 * 3 * C_  # workgroups x waves (8; 4 with LNX_CM_NW=4 at C = 192) x (2C + C)
    ws = torch.empty(need, device="cuda")

    def run(init):
        dgam, dw, db = init((C_,)), init((C_,)), init((C_,))
        ops.convmlp_bwd(gout, ln, z, w1, b1, w2t, w1t, gam, e(M, 4 * C_), e(M, 4 * C_), e(M, C_), e(M, C_), dgam, rowscale=rs, rows_per_sample=rps, y=y,
                        ln_w=lw, mean=mean, rstd=rstd, d_ln_w=dw, d_ln_b=db, ws=ws)
        return [dgam, dw, db]

    check_case(run, refs, [1e-3, 3e-3, 3e-3], [1e-2, 3e-3, 3e-3], load, scales=[rms(sd * gout.double().cpu() * z.double().cpu()), rms(dl * xh), rms(dl)])
    # the scratch of the default mode (a row per workgroup) is too small for a row per wave: refused by name, nothing overrun
    linnaeus_amd.set_deterministic(True)
    small = torch.empty(need // 12, device="cuda")
    with pytest.raises(L.LnxError, match="lnx_convmlp_bwd: ws too small"):
        ops.convmlp_bwd(gout, ln, z, w1, b1, w2t, w1t, gam, None, None, e(M, C_), e(M, C_), torch.zeros(C_, device="cuda"), rowscale=rs, rows_per_sample=rps,
                        y=y, ln_w=lw, mean=mean, rstd=rstd, d_ln_w=torch.zeros(C_, device="cuda"), d_ln_b=torch.zeros(C_, device="cuda"), ws=small)
