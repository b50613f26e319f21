"""DropPath compaction of the conv blocks: the depthwise kernels with a list (lnx_dwconv7_fwd_kept / lnx_dwconv7_wgrad_kept), the fused
conv-MLP kernels on compact rows (lnx_convmlp_args::perm / m_dev), and the model with the switch on against off.

The idiom of tests/test_gpu_droppath_compact.py: NaN in every row a kernel must not read, a sentinel in every row it must not write, and
its PATTERNS of multipliers.  Compact row m' of a call is sample perm[m' // rps], pixel m' % rps; rows >= m_eff = nkeep * rps are nobody's.
The fp32 streams (x / out, g) and the depthwise kernels' tensors (y, dln) keep natural sample order; ln, mean, rstd, act, dh, dz are compact."""
import numpy as np
import pytest
import torch

import linnaeus_amd
from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests.test_gpu_droppath_compact import PATTERNS, SENTINEL, _i32, _partition_ref, _pattern

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
NAN = float("nan")


@pytest.fixture(autouse=True)
def _switches_back():
    yield
    linnaeus_amd.set_deterministic(False)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _lists(sc, rps):
    lists = ops.drop_partition(torch.from_numpy(sc[None]).cuda(), rows_per_sample=[rps])
    perm, nkeep, _ = _partition_ref(sc)
    return lists, perm, nkeep


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. depthwise forward, data gradient and weight gradient with a list
# ---------------------------------------------------------------------------------------------------------------------------------
# route -> (x dtype of forward / weight gradient, y dtype of the forward, dy dtype): the matrix-core kernels as the plan calls them, and the
# fp32 VALU kernels
ROUTES = {"mfma": (torch.float32, BF, BF), "valu": (torch.float32, torch.float32, torch.float32)}


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("HW", [7, 16])  # 16: two 14-pixel tiles per axis with a ragged edge
@pytest.mark.parametrize("route", list(ROUTES))
def test_depthwise_with_a_list(route, HW, pattern):
    xdt, ydt, dydt = ROUTES[route]
    B, C_ = 5, 96
    rng = np.random.default_rng(HW * 7 + PATTERNS.index(pattern))
    sc = _pattern(pattern, B, rng)
    lists, perm, nkeep = _lists(sc, HW * HW)
    kept, dropped = torch.from_numpy(perm[:nkeep]).long().cuda(), torch.from_numpy(perm[nkeep:]).long().cuda()
    g = torch.Generator().manual_seed(HW + B)
    x0 = torch.randn(B, HW, HW, C_, generator=g).cuda().to(xdt)
    w49 = (0.2 * torch.randn(49, C_, generator=g)).cuda()
    bias = (0.1 * torch.randn(C_, generator=g)).cuda()
    kw = dict(perm=lists.perm(0), nkeep=lists.nkeep(0))

    # forward: kept samples as without a list, dropped samples' y not written, their x not read
    ref = torch.empty(B, HW, HW, C_, device="cuda", dtype=ydt)
    ops.dwconv7(x0, w49, bias, ref)
    x = x0.clone()
    x[dropped] = NAN
    y = torch.full((B, HW, HW, C_), SENTINEL, device="cuda", dtype=ydt)
    ops.dwconv7(x, w49, bias, y, **kw)
    torch.cuda.synchronize()
    assert not torch.isnan(y.float()).any()
    assert _same_bits(y[kept], ref[kept]), "forward: kept samples"
    assert torch.equal(y[dropped], torch.full_like(y[dropped], SENTINEL)), "forward: dropped samples were written"

    # data gradient (flipped kernel, res = y = g in place): kept samples as without a list, g of dropped samples unchanged
    dy0 = torch.randn(B, HW, HW, C_, generator=g).cuda().to(dydt)
    g0 = torch.randn(B, HW, HW, C_, generator=g).cuda()
    gref = g0.clone()
    ops.dwconv7(dy0, w49, None, gref, flip=True, res=gref)
    dy = dy0.clone()
    dy[dropped] = NAN
    gg = g0.clone()
    gg[dropped] = SENTINEL
    ops.dwconv7(dy, w49, None, gg, flip=True, res=gg, **kw)
    torch.cuda.synchronize()
    assert not torch.isnan(gg).any()
    assert _same_bits(gg[kept], gref[kept]), "data gradient: kept samples"
    assert torch.equal(gg[dropped], torch.full_like(gg[dropped], SENTINEL)), "data gradient: g of dropped samples was touched"

    # weight gradient: that of the gathered kept batch -- within test_dwconv_mfma's bound, and bit for bit in deterministic mode
    for det in (False, True):
        linnaeus_amd.set_deterministic(det)
        dw, db = torch.zeros(C_, 1, 7, 7, device="cuda"), torch.zeros(C_, device="cuda")
        ops.dwconv7_wgrad(x, dy, dw, db, **kw)
        torch.cuda.synchronize()
        assert not torch.isnan(dw).any() and not torch.isnan(db).any()
        if nkeep == 0:
            assert not dw.any() and not db.any()
            continue
        dwg, dbg = torch.zeros_like(dw), torch.zeros_like(db)
        ops.dwconv7_wgrad(x0[kept].contiguous(), dy0[kept].contiguous(), dwg, dbg)
        if det:
            assert torch.equal(dw, dwg) and torch.equal(db, dbg), "deterministic mode: the gathered batch's bits"
            dw2, db2 = torch.zeros_like(dw), torch.zeros_like(db)
            ops.dwconv7_wgrad(x, dy, dw2, db2, **kw)
            assert torch.equal(dw, dw2) and torch.equal(db, db2), "deterministic mode: run to run"
        else:
            sc_ = (B * HW * HW) ** 0.5
            torch.testing.assert_close(dw, dwg, rtol=1e-4, atol=2e-5 * sc_)
            torch.testing.assert_close(db, dbg, rtol=1e-4, atol=2e-5 * sc_)
    linnaeus_amd.set_deterministic(False)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. conv-MLP forward and backward on compact rows
# ---------------------------------------------------------------------------------------------------------------------------------
def _mlp_cases():
    """(B, rps, multipliers): sample seams inside a row tile (49, 196 rows per sample) under every pattern, and 64 rows per sample with
    0, 2 and 4 samples kept -- m_eff = 0 or on a tile edge (16-, 32- and 128-row tiles)"""
    for i, name in enumerate(PATTERNS):
        yield f"49-{name}", 5 + i % 3, 49, _pattern(name, 5 + i % 3, np.random.default_rng(40 + i))
    for name in ("first_only", "random", "odd_values"):
        yield f"196-{name}", 6, 196, _pattern(name, 6, np.random.default_rng(len(name)))
    for nkeep in (0, 2, 4):
        sc = np.zeros(7, dtype=np.float32)
        sc[[5, 1, 6, 3][:nkeep]] = 1.25
        yield f"64-keep{nkeep}", 7, 64, sc


MLP_CASES = list(_mlp_cases())


def _ws(C_, M):
    return torch.full((max(int(L.lib().lnx_convmlp_bwd_ws_floats(C_, M)), 1),), NAN, device="cuda")


@pytest.mark.parametrize("case", MLP_CASES, ids=[c[0] for c in MLP_CASES])
@pytest.mark.parametrize("C_", [96, 192])  # resident weights / streamed weights
def test_convmlp_on_compact_rows(C_, case):
    """The forms a training plan launches (LayerNorm inside, no z: the LayerScale gradient comes from the pwconv2 weight gradient, so
    dgamma is not produced by these calls and z is refused together with a list)."""
    _, B, rps, sc = case
    M = B * rps
    lists, perm, nkeep = _lists(sc, rps)
    m_eff = nkeep * rps
    perm_t = torch.from_numpy(perm).long().cuda()
    rows_c = (perm_t[:, None] * rps + torch.arange(rps, device="cuda")[None]).reshape(M)  # natural row of every compact row
    kept_rows, drop_rows = rows_c[:m_eff], rows_c[m_eff:]
    gen = torch.Generator().manual_seed(C_ + M)
    y0 = (1.5 * torch.randn(M, C_, generator=gen) + 0.3).cuda().to(BF)
    lw = (1.0 + 0.2 * torch.randn(C_, generator=gen)).cuda()
    lb = (0.1 * torch.randn(C_, generator=gen)).cuda()
    w1 = (torch.randn(4 * C_, C_, generator=gen) / C_**0.5).cuda().to(BF)
    b1 = (0.2 * torch.randn(4 * C_, generator=gen)).cuda()
    w2 = (torch.randn(C_, 4 * C_, generator=gen) / (4 * C_) ** 0.5).cuda().to(BF)
    b2 = (0.2 * torch.randn(C_, generator=gen)).cuda()
    gam = (0.5 + 0.3 * torch.randn(C_, generator=gen)).cuda()
    x = torch.randn(M, C_, generator=gen).cuda()
    g0 = torch.randn(M, C_, generator=gen).cuda()
    rs = torch.from_numpy(sc).cuda()
    w2t, w1t = w2.t().contiguous(), w1.t().contiguous()
    lnkw = dict(ln_w=lw, ln_b=lb, ln_eps=1e-6)
    kw = dict(perm=lists.perm(0), m_dev=lists.m_dev(0))

    def full(shape, dt=torch.float32, v=SENTINEL):
        return torch.full(shape, v, device="cuda", dtype=dt)

    # ---- forward.  References: the full-row call with the same multipliers, and the call on the gathered kept rows
    out_f, ln_f, mean_f, rstd_f = full((M, C_)), full((M, C_), BF), full((M,)), full((M,))
    ops.convmlp_fwd(None, w1, b1, w2, b2, gam, x, out_f, rowscale=rs, rows_per_sample=rps, y=y0, ln_out=ln_f, mean=mean_f, rstd=rstd_f, **lnkw)
    if m_eff:
        rs_g = rs[perm_t[:nkeep]].contiguous()
        y_g, x_g = y0[kept_rows].contiguous(), x[kept_rows].contiguous()
        out_g, ln_g, mean_g, rstd_g = full((m_eff, C_)), full((m_eff, C_), BF), full((m_eff,)), full((m_eff,))
        ops.convmlp_fwd(None, w1, b1, w2, b2, gam, x_g, out_g, rowscale=rs_g, rows_per_sample=rps, y=y_g, ln_out=ln_g, mean=mean_g, rstd=rstd_g, **lnkw)
    y = y0.clone()
    y[drop_rows] = NAN  # the depthwise forward does not write the dropped samples' rows
    out, ln, mean, rstd = full((M, C_)), full((M, C_), BF), full((M,)), full((M,))
    ops.convmlp_fwd(None, w1, b1, w2, b2, gam, x, out, rowscale=rs, rows_per_sample=rps, y=y, ln_out=ln, mean=mean, rstd=rstd, **lnkw, **kw)
    torch.cuda.synchronize()
    for t in (out, ln, mean, rstd):
        assert not torch.isnan(t.float()).any()
    assert _same_bits(out[kept_rows], out_f[kept_rows]), "out: kept rows against the full-row call"
    assert _same_bits(out[drop_rows], x[drop_rows]), "out: rows of dropped samples are x"
    for name, got, sent in (("ln", ln, ln_f), ("mean", mean, mean_f), ("rstd", rstd, rstd_f)):
        assert torch.equal(got[m_eff:], torch.full_like(got[m_eff:], SENTINEL)), f"{name}: rows >= m_eff were written"
        assert _same_bits(got[:m_eff], sent[kept_rows]), f"{name}: compact rows against the full-row call's"
    if m_eff:
        assert _same_bits(out[kept_rows], out_g) and _same_bits(ln[:m_eff], ln_g) and _same_bits(mean[:m_eff], mean_g) and _same_bits(rstd[:m_eff], rstd_g), \
            "compact rows against the gathered call"
    # the inference form of the call (no LayerNorm outputs) takes a list as well
    out2 = full((M, C_))
    ops.convmlp_fwd(None, w1, b1, w2, b2, gam, x, out2, rowscale=rs, rows_per_sample=rps, y=y, **lnkw, **kw)
    assert _same_bits(out2, out)

    # ---- backward, immediate and deferred fold of the LayerNorm column sums
    def bwd(Mr, g, ln_, y_, mean_, rstd_, rs_, defer, **extra):
        act, dh, dz = full((Mr, 4 * C_), BF), full((Mr, 4 * C_), BF), full((Mr, C_), BF)
        dln = full((g.shape[0], C_), BF)
        dlw, dlb = full((C_,), v=3.0), full((C_,), v=-2.0)  # accumulated into
        ws = _ws(C_, g.shape[0])
        ops.convmlp_bwd(g, ln_, None, w1, b1, w2t, w1t, gam, act, dh, dz, dln, None, rowscale=rs_, rows_per_sample=rps, y=y_, ln_w=lw, mean=mean_,
                        rstd=rstd_, d_ln_w=dlw, d_ln_b=dlb, ws=ws, dz_plain=True, ln_defer=defer, **extra)
        if defer:
            ops.layernorm_bwd_flush()
        torch.cuda.synchronize()
        return act, dh, dz, dln, dlw - 3.0, dlb + 2.0

    ln_in, mean_in, rstd_in = ln.clone(), mean.clone(), rstd.clone()
    for t in (ln_in, mean_in, rstd_in):
        t[m_eff:] = NAN
    g = g0.clone()
    g[drop_rows] = NAN  # the gradient of a dropped sample is neither read nor written
    g_before = _bits(g).clone()
    for defer in (False, True):
        act, dh, dz, dln, dlw, dlb = bwd(M, g, ln_in, y, mean_in, rstd_in, rs, defer, **kw)
        assert torch.equal(_bits(g), g_before), "g was written"
        for name, t in (("act", act), ("dh", dh), ("dz", dz)):
            assert not torch.isnan(t.float()).any(), name
            assert torch.equal(t[m_eff:], torch.full_like(t[m_eff:], SENTINEL)), f"{name}: rows >= m_eff were written"
        assert not torch.isnan(dln.float()).any() and not torch.isnan(dlw).any() and not torch.isnan(dlb).any()
        assert torch.equal(dln[drop_rows], torch.full_like(dln[drop_rows], SENTINEL)), "dln: rows of dropped samples were written"
        if not m_eff:
            assert not dlw.any() and not dlb.any()
            continue
        act_g, dh_g, dz_g, dln_g, dlw_g, dlb_g = bwd(m_eff, g0[kept_rows].contiguous(), ln_g, y_g, mean_g, rstd_g, rs_g, defer)
        assert _same_bits(act[:m_eff], act_g) and _same_bits(dh[:m_eff], dh_g) and _same_bits(dz[:m_eff], dz_g), "compact rows against the gathered call"
        assert _same_bits(dln[kept_rows], dln_g), "dln: kept samples against the gathered call"
        # the column sums: the bound test_convmlp_fused_layernorm holds two launches of one kernel to (another summation order)
        scale = max(1.0, dlw_g.abs().max().item())
        torch.testing.assert_close(dlw, dlw_g, rtol=1e-5, atol=1e-4 * scale)
        torch.testing.assert_close(dlb, dlb_g, rtol=1e-5, atol=1e-4 * max(1.0, dlb_g.abs().max().item()))

    # a list together with z is refused by name
    with pytest.raises(L.LnxError):
        ops.convmlp_fwd(None, w1, b1, w2, b2, gam, x, out2, rowscale=rs, rows_per_sample=rps, y=y, ln_out=ln, mean=mean, rstd=rstd, z=full((M, C_), BF), **lnkw, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. - 5. the model
# ---------------------------------------------------------------------------------------------------------------------------------
from tests.cases import load_case  # noqa: E402
from tests.test_gpu_droppath_compact import _injections  # noqa: E402
from tests.test_gpu_model import _grads, build, run as run_model  # noqa: E402


def _conv_injections(spec, B, drops):
    """hand-made multipliers of the conv calls in front of the RoPE calls' hand-made ones: (a) one conv call fully kept, one fully dropped,
    the last sample dropped in the third; (b) sample 0 dropped in two consecutive blocks, the last sample dropped in the third"""
    n_conv = sum(spec.conv_depths)
    assert n_conv == 3
    rope = _injections(spec, B, drops)["hand"][n_conv:]
    keep = torch.full((B,), 1.25)
    first, last, none = keep.clone(), keep.clone(), torch.zeros(B)
    first[0] = 0.0
    last[-1] = 0.0
    return {"kept_dropped_last": [keep, none, last] + rope, "sample0_twice_last": [first, first.clone(), last] + rope}


@pytest.mark.parametrize("ckpt", [False, True])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["tiny_b", "tiny_dp"])
def test_model_switch_on_equals_switch_off(name, dtype, ckpt, golden_dir, monkeypatch):
    """The conv counter advances exactly when the switch is on and the conv blocks run fused with the LayerNorm inside: the bf16 plans
    (the fp32 plans' conv blocks run unfused: part of the gate)."""
    from oracle import mformer_oracle as O
    spec, z, sd, x, meta, drops = load_case(name, golden_dir)
    model = build(name, spec, sd, dtype)
    B = x.shape[0]
    xs, ms = x.cuda(), meta.cuda() if meta is not None else None

    def step(inj):
        model.zero_grad(set_to_none=True)
        model.train(True)
        model._inject_drop = inj
        conv0, rope0 = model.drop_compact_conv_blocks(), model.drop_compact_branches()
        out = model(xs, ms, force_checkpointing=True) if ckpt else model(xs, ms)
        feats = model._last_feats.detach().clone()
        O.probe_loss(out).backward()
        return ({k: v.detach().clone() for k, v in out.items()}, feats, _grads(model)), model.drop_compact_conv_blocks() - conv0, model.drop_compact_branches() - rope0

    try:
        for tag, inj in _conv_injections(spec, B, drops).items():
            res = {}
            for on in (False, True):
                model.set_drop_compact(on)
                res[on], conv_ran, rope_ran = step(inj)
                assert (conv_ran > 0) == (on and dtype == "bf16"), (tag, on, conv_ran)
                assert (rope_ran > 0) == on, (tag, on, rope_ran)
            for t in res[True][0]:
                assert torch.equal(res[True][0][t], res[False][0][t]), (tag, t)
            assert torch.equal(res[True][1], res[False][1]), tag
            osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
            O.probe_loss(O.forward(osd, spec, x, meta, inj)).backward()
            worst_d = 0.0
            for k, p_ in model.named_parameters():  # test_backward_matches_oracle's bounds
                parts = k.split(".")
                ck = f"head.{parts[3]}.fc.{parts[4]}" if (parts[0] == "head" and len(parts) >= 5 and parts[2] == "level_classifiers") else k
                ref = osd[ck].grad
                got = res[True][2][k].float().cpu()
                denom = max(ref.norm().item(), 1e-3 * (1 if dtype == "fp32" else 10))
                tol = 2e-3 if dtype == "fp32" else (0.25 if ck.startswith("meta_") else 0.10)
                assert (got - ref).norm().item() <= tol * denom, (tag, k, (got - ref).norm().item(), denom)
                worst_d = max(worst_d, (res[True][2][k].float() - res[False][2][k].float()).norm().item() / denom)
            print(f"[{name}/{dtype}/ckpt={ckpt}/{tag}] worst on/off gradient difference relative to the oracle's norm: {worst_d:.3e}")
            # the conv part alone switched off: the RoPE counter advances, the conv counter stands still, same logits
            model.set_drop_compact(True)
            monkeypatch.setenv("LNX_DROP_COMPACT_CONV", "0")
            part, conv_ran, rope_ran = step(inj)
            monkeypatch.delenv("LNX_DROP_COMPACT_CONV")
            assert conv_ran == 0 and rope_ran > 0, (tag, conv_ran, rope_ran)
            for t in part[0]:
                assert torch.equal(part[0][t], res[True][0][t]), (tag, t)
    finally:
        model.set_drop_compact(None)


def test_gates_keep_the_conv_blocks_on_full_rows(golden_dir, monkeypatch):
    from linnaeus_amd import build_model
    from oracle import mformer_oracle as O
    from tests.cases import make_config, model_state_dict_from_oracle
    spec, z, sd, x, meta, drops = load_case("tiny_dp", golden_dir)
    inj = _conv_injections(spec, x.shape[0], drops)["sample0_twice_last"]
    n = len(O.drop_call_probs(spec))
    model = build("tiny_dp", spec, sd, "bf16")

    def moved(m, drops_, train=True):
        before = m.drop_compact_conv_blocks()
        out = run_model(m, x, meta, drops_, train=train)
        if train:
            O.probe_loss(out).backward()
        return m.drop_compact_conv_blocks() - before

    assert moved(model, inj) > 0                       # (the gates below are closed one at a time from this open state)
    assert moved(model, [None] * n) == 0               # no drop pointer
    with torch.no_grad():
        assert moved(model, None, train=False) == 0    # an inference plan
    fp32 = build("tiny_dp", spec, sd, "fp32")         # conv blocks that run unfused
    assert moved(fp32, inj) == 0
    monkeypatch.setenv("LNX_NO_FUSED_LN", "1")          # ... or fused without the LayerNorm inside
    assert moved(build("tiny_dp", spec, sd, "bf16"), inj) == 0
    monkeypatch.delenv("LNX_NO_FUSED_LN")
    cfg = make_config(spec, 64)                          # DROP_RATE > 0: the dropout masks are laid out by full rows
    cfg.MODEL.DROP_RATE = 0.2
    dr = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    dr.load_state_dict(model_state_dict_from_oracle(dr, sd), strict=True)
    dr = dr.cuda()
    dr.set_compute_dtype("bf16")
    assert moved(dr, inj) == 0
    assert all(torch.isfinite(p_.grad).all() for p_ in dr.parameters())


@pytest.mark.parametrize("ckpt", [False, True])
def test_deterministic_steps_with_the_conv_compaction(ckpt, golden_dir):
    from oracle import mformer_oracle as O
    spec, z, sd, x, meta, drops = load_case("tiny_dp", golden_dir)
    model = build("tiny_dp", spec, sd, "bf16")
    model.set_deterministic(True)
    inj = _conv_injections(spec, x.shape[0], drops)["sample0_twice_last"]
    xs, ms = x.cuda(), meta.cuda() if meta is not None else None
    runs = []
    try:
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            model.train(True)
            model._inject_drop = inj
            before = model.drop_compact_conv_blocks()
            out = model(xs, ms, force_checkpointing=True) if ckpt else model(xs, ms)
            O.probe_loss(out).backward()
            torch.cuda.synchronize()
            assert model.drop_compact_conv_blocks() > before
            runs.append(({k: v.detach().clone() for k, v in out.items()}, _grads(model)))
    finally:
        model.set_deterministic(False)
    for t in runs[0][0]:
        assert torch.equal(runs[0][0][t], runs[1][0][t]), t
    diff = [k for k in runs[0][1] if not torch.equal(runs[0][1][k], runs[1][1][k])]
    assert not diff, f"{len(diff)} gradients differ between two deterministic steps, e.g. {diff[:6]}"
