"""The CLS-only last RoPE block (LNX_LAST_CLS / lnx_set_last_cls): norm_2 reads the CLS row of the stage-4 output
and nothing else, so the last stage-4 block runs proj, LayerNorm 2, fc1 and fc2 -- forward and backward -- on the batch's CLS rows.

Switch on against switch off on the same weights, inputs and injected DropPath multipliers, both against the fp32 oracle inside the
bounds tests/test_gpu_model.py applies to the same quantities:
    logits   fp32 rtol 1e-4 / atol 1e-4 x scale, bf16 max|err| <= 0.025 x scale          (test_sm_b24_production_dispatch_matches_oracle)
    loss     fp32 |err| < 2e-4 x max(1, |loss|)                                            (test_backward_matches_oracle)
    grads    per parameter ||err|| <= tol x max(||ref||, floor): fp32 2e-3 (floor 1e-3), bf16 0.10, metadata heads 0.25 (floor 1e-2);
             whole gradient fp32 1e-3, bf16 5e-2                                           (test_backward_matches_oracle)
The on / off bound is three times the largest off-against-off difference measured by measure_off_against_off() below (default mode,
where split contractions and LayerNorm column sums meet in float atomics); see ONOFF."""
import ctypes as C

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from oracle import mformer_oracle as O
from tests.cases import CASES, HEADS2, TINY_DIMS, make_config, model_state_dict_from_oracle
from tests.test_gpu_model import _drop_scales, _grads

pytestmark = pytest.mark.gpu

# two stage-4 blocks (the last one follows another block) and tiny_dp's one (first and last of its stage at once)
SPECS = {
    "two": O.Spec(conv_dims=TINY_DIMS, conv_depths=(1, 1), rope_depths=(1, 2), rope_heads=(2, 4), heads=HEADS2, drop_path_rate=0.5),
    "one": CASES["tiny_dp"],
}
IMG = 64
DRAWS = ("sample0", "kept", "dropped")

# Off against off, measured by measure_off_against_off() on an MI355X in the default (atomic) mode: per storage type the largest figure
# of each quantity, as _diff() defines them, over every (spec, B, draw) of test_on_equals_off (two runs of the full block each), and
# for the production case over four runs of it.  The bound on on-against-off is three times that.
#   tiny, fp32: logits 0, loss 0 (bit-equal run to run), gradients 3.28e-6      (on against off, same session: 0, 0, 7.94e-7)
#   tiny, bf16: logits 0, loss 0,                        gradients 4.08e-7      (on against off: 0, 0, 2.03e-7)
#   sm @224, B = 8, bf16: logits 0, loss 0,            gradients 3.13e-7      (on against off: 0, 0, 2.74e-7)
# (A second session measured 4.83e-6 / 1.05e-6 for the tiny cases: the figure is itself noise.  The smaller, first one is kept.)
# Logits and loss: the forward has no atomics, so two runs agree bit for bit and the bound is 0 -- on against off must be bit-equal as
# well, and is: with a DropPath multiplier the CLS rows' proj / fc1 / fc2 take the same 128x128 kernel as the full block's rows at
# these sizes, and a row's K loop does not depend on which rows share its tile.
OFF_OFF = {"fp32": {"logits": 0.0, "loss": 0.0, "grads": 3.28e-6}, "bf16": {"logits": 0.0, "loss": 0.0, "grads": 4.08e-7},
           "sm_b8_bf16": {"logits": 0.0, "loss": 0.0, "grads": 3.13e-7}}
ONOFF = {dt: {k: 3.0 * v for k, v in d.items()} for dt, d in OFF_OFF.items()}


def _model(spec, sd, dtype, img=IMG, **cfg_over):
    cfg = make_config(spec, img)
    for k, v in cfg_over.items():
        setattr(cfg.MODEL, k, v)
    model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype(dtype)
    return model


def _inject(spec, B, draw, seed=31):
    """The seeded draw of every call, with the last stage-4 block's two calls (the last two of the list) set by hand."""
    inj = _drop_scales(spec, B, seed)
    for j in (-2, -1):
        keep = 1.0 - O.drop_call_probs(spec)[j]
        v = torch.full((B,), 1.0 / keep)
        if draw == "sample0":
            v[0] = 0.0
        elif draw == "dropped":
            v[:] = 0.0
        inj[j] = v
    return inj


def _step(model, x, meta, inj, on, ckpt=False):
    """One training forward + backward of the probe loss under the switch: logits, loss, gradients, and how many block forwards ran CLS-only."""
    model.set_last_cls(on)
    model.zero_grad(set_to_none=True)
    model.train(True)
    model._inject_drop = inj
    before = model.last_cls_blocks()
    out = model(x, meta, force_checkpointing=True) if ckpt else model(x, meta)
    loss = O.probe_loss(out)
    loss.backward()
    torch.cuda.synchronize()
    return {k: v.detach().float().clone() for k, v in out.items()}, float(loss.item()), _grads(model), model.last_cls_blocks() - before


def _floor(dtype):
    return 1e-3 * (1 if dtype == "fp32" else 10)


def _diff(a, b, dtype):
    """(logits, loss, gradients): max|d logits| / max(1, max|logits|), |d loss| / max(1, |loss|), worst per-parameter ||d g|| / max(||g||, floor)"""
    dl = max((a[0][t] - b[0][t]).abs().max().item() / max(1.0, b[0][t].abs().max().item()) for t in b[0])
    ds = abs(a[1] - b[1]) / max(1.0, abs(b[1]))
    dg = max((a[2][k].float() - b[2][k].float()).norm().item() / max(b[2][k].float().norm().item(), _floor(dtype)) for k in b[2])
    return {"logits": dl, "loss": ds, "grads": dg}


def _oracle(spec, sd, x, meta, inj):
    osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    out = O.forward(osd, spec, x, meta, inj)
    loss = O.probe_loss(out)
    loss.backward()
    return {t: v.detach() for t, v in out.items()}, float(loss.item()), {k: v.grad for k, v in osd.items()}


def _assert_oracle(res, ref, dtype, tag):
    """tests/test_gpu_model.py's bounds, quoted in the module docstring"""
    logits, loss, grads = res[0], res[1], res[2]
    for t, r in ref[0].items():
        got = logits[t].cpu()
        scale = max(1.0, r.abs().max().item())
        if dtype == "fp32":
            torch.testing.assert_close(got, r, rtol=1e-4, atol=1e-4 * scale, msg=f"{tag} {t}")
        else:
            assert (got - r).abs().max().item() <= 0.025 * scale, (tag, t)
    if dtype == "fp32":
        assert abs(loss - ref[1]) < 2e-4 * max(1.0, abs(ref[1])), (tag, loss, ref[1])
    tot_err = tot_ref = 0.0
    for k, g in grads.items():
        parts = k.split(".")
        ck = f"head.{parts[3]}.fc.{parts[4]}" if (parts[0] == "head" and len(parts) >= 5 and parts[2] == "level_classifiers") else k
        r = ref[2][ck]
        err, denom = (g.float().cpu() - r).norm().item(), r.norm().item()
        tot_err += err * err
        tot_ref += denom * denom
        tol = 2e-3 if dtype == "fp32" else (0.25 if ck.startswith("meta_") else 0.10)
        assert err <= tol * max(denom, _floor(dtype)), (tag, k, err, denom)
    assert (tot_err / tot_ref) ** 0.5 <= (1e-3 if dtype == "fp32" else 5e-2), tag


def _case(which, B, seed=5):
    spec = SPECS[which]
    sd = O.seeded_state_dict(O.param_shapes(spec), 900 + seed)
    x, meta = O.seeded_inputs(spec, B, IMG, 901 + seed)
    return spec, sd, x, meta


def _prod_case(B=8):
    spec = O.Spec(heads=(("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20)), drop_path_rate=0.2)
    sd = O.seeded_state_dict(O.param_shapes(spec), 777)
    x, meta = O.seeded_inputs(spec, B, 224, 778)
    return spec, sd, x, meta, _inject(spec, B, "sample0", seed=779)


def measure_off_against_off():
    """Prints, per dtype, the largest off-against-off figures over test_on_equals_off's cases (two runs of the full block, default mode)."""
    for dtype in ("fp32", "bf16"):
        worst = {"logits": 0.0, "loss": 0.0, "grads": 0.0}
        for which in SPECS:
            for B in (3, 17):
                spec, sd, x, meta = _case(which, B)
                model = _model(spec, sd, dtype)
                xs, ms = x.cuda(), meta.cuda()
                for draw in DRAWS:
                    inj = _inject(spec, B, draw)
                    a, b = _step(model, xs, ms, inj, False), _step(model, xs, ms, inj, False)
                    on = _step(model, xs, ms, inj, True)
                    d, e = _diff(a, b, dtype), _diff(on, b, dtype)
                    print(f"[measure {dtype} {which} B={B} {draw}] off/off {d}  on/off {e}", flush=True)
                    worst = {k: max(worst[k], d[k]) for k in worst}
                model.set_last_cls(None)
        print(f"[measure {dtype}] worst off against off: {worst}", flush=True)
    spec, sd, x, meta, inj = _prod_case()
    model = _model(spec, sd, "bf16", img=224)
    xs, ms = x.cuda(), meta.cuda()
    runs = [_step(model, xs, ms, inj, False) for _ in range(4)]
    on = _step(model, xs, ms, inj, True)
    model.set_last_cls(None)
    worst = {"logits": 0.0, "loss": 0.0, "grads": 0.0}
    for i in range(len(runs)):
        for j in range(i):
            d = _diff(runs[i], runs[j], "bf16")
            worst = {k: max(worst[k], d[k]) for k in worst}
    print(f"[measure sm B=8 bf16] worst off against off over {len(runs)} runs: {worst}  on/off {_diff(on, runs[0], 'bf16')}", flush=True)


@pytest.mark.parametrize("B", [3, 17])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("which", ["two", "one"])
def test_on_equals_off(which, dtype, B):
    """Logits, loss and every parameter gradient, name by name, with the path on and off: the last block's sample 0 dropped, every sample
    kept, every sample dropped.  Both runs inside the oracle bounds; on against off inside ONOFF.

    Measured (MI355X, measure_off_against_off): off against off logits 0, loss 0, gradients <= 3.28e-6 (fp32) / 4.08e-7 (bf16) of the
    parameter's gradient norm; on against off in the same session logits 0, loss 0, gradients <= 7.94e-7 (fp32) / 2.03e-7 (bf16).  The
    bound is three times the off-against-off figure: 0, 0, 9.84e-6 / 1.22e-6."""
    spec, sd, x, meta = _case(which, B)
    model = _model(spec, sd, dtype)
    xs, ms = x.cuda(), meta.cuda()
    try:
        for draw in DRAWS:
            inj = _inject(spec, B, draw)
            ref = _oracle(spec, sd, x, meta, inj)
            off, on = _step(model, xs, ms, inj, False), _step(model, xs, ms, inj, True)
            assert off[3] == 0 and on[3] == 1, (draw, off[3], on[3])
            _assert_oracle(off, ref, dtype, f"{draw} off")
            _assert_oracle(on, ref, dtype, f"{draw} on")
            d = _diff(on, off, dtype)
            print(f"[{which}/{dtype}/B={B}/{draw}] on against off: {d}")
            for k, v in d.items():
                assert v <= ONOFF[dtype][k], (draw, k, v, ONOFF[dtype][k])
    finally:
        model.set_last_cls(None)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_deterministic_mode_on_against_on_is_bit_equal(dtype):
    spec, sd, x, meta = _case("two", 17)
    model = _model(spec, sd, dtype)
    xs, ms = x.cuda(), meta.cuda()
    inj = _inject(spec, 17, "sample0")
    model.set_deterministic(True)
    try:
        for on in (False, True):
            a, b = _step(model, xs, ms, inj, on), _step(model, xs, ms, inj, on)
            assert a[3] == (1 if on else 0)
            assert all(torch.equal(a[0][t], b[0][t]) for t in a[0]) and a[1] == b[1], on
            for k in a[2]:
                assert torch.equal(a[2][k], b[2][k]), (on, k)
    finally:
        model.set_deterministic(False)
        model.set_last_cls(None)


def test_production_dispatch_sm_b8_bf16():
    """sm @224, B = 8, bf16: the full block's proj / fc1 / fc2 run on 416 rows, the CLS-only ones on 8 -- the one-wave and 128x128 kernels
    (tests/test_last_cls_host.py states which product takes which).  Same comparisons as above; the kernels are read off the
    dispatcher's own record.  Measured: off against off over four runs logits 0, loss 0, gradients 3.13e-7; on against off 0, 0,
    2.74e-7; the bound is three times the former: 0, 0, 9.39e-7."""
    B, dtype = 8, "bf16"
    spec, sd, x, meta, inj = _prod_case()
    ref = _oracle(spec, sd, x, meta, inj)
    model = _model(spec, sd, dtype, img=224)
    xs, ms = x.cuda(), meta.cuda()
    lib = L.lib()
    try:
        res, launches = {}, {}
        for on in (False, True):
            n0 = [lib.lnx_nt_kernel_launches(k) for k in (L.NT_KERNEL_V1, L.NT_KERNEL_SKINNY)]
            res[on] = _step(model, xs, ms, inj, on)
            launches[on] = [lib.lnx_nt_kernel_launches(k) - n for k, n in zip((L.NT_KERNEL_V1, L.NT_KERNEL_SKINNY), n0)]
            _assert_oracle(res[on], ref, dtype, f"on={on}")
        assert res[False][3] == 0 and res[True][3] == 1
        # The full block's six products (416 rows, below the tile kernels' 1024) are six launches of the 128x128 kernel.  CLS-only: proj,
        # fc1, fc2 forward and the fc2 data gradient (row scale / two outputs / GELU' epilogues) stay on it with 8 rows, and so does the
        # proj data gradient here (the attention call has a DropPath list, and the one-wave kernel takes no device row count); the
        # plain fc1 data gradient moves to the one-wave kernel -- one launch fewer of the one, one more of the other
        assert launches[True][0] - launches[False][0] == -1 and launches[True][1] - launches[False][1] == 1, launches
        for N, K in ((768, 3072), (3072, 768), (768, 768)):
            q = L.TnLaunch()
            a = L.WgradArgs()
            a.dtype, a.M, a.N, a.K, a.lddy, a.lda = L.BF16, B, N, K, N, K
            assert lib.lnx_gemm_tn_query(C.byref(a), C.byref(q)) == 0 and (q.kernel, q.splits, q.workspace) == (L.TN_KERNEL_V1, 1, 0)
        d = _diff(res[True], res[False], dtype)
        print(f"[sm B=8 bf16] on against off: {d}")
        for k, v in d.items():
            assert v <= ONOFF["sm_b8_bf16"][k], (k, v, ONOFF["sm_b8_bf16"][k])
    finally:
        model.set_last_cls(None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the other plans
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,dtype", [("two", "fp32"), ("one", "bf16")])
def test_recompute_plan_equals_kept_activations_with_the_path_on(which, dtype):
    """test_recompute_plan_equals_kept_activations' property: same logits bit for bit, gradients within 1e-5 of their norm."""
    spec, sd, x, meta = _case(which, 3)
    model = _model(spec, sd, dtype)
    xs, ms = x.cuda(), meta.cuda()
    inj = _inject(spec, 3, "sample0")
    try:
        a, b = _step(model, xs, ms, inj, True), _step(model, xs, ms, inj, True, ckpt=True)
        assert any(k[-1] for k in model._plans), "no recompute plan was created"
        assert a[3] == 1 and b[3] >= 1
        for t in a[0]:
            assert torch.equal(a[0][t], b[0][t]), t
        for k in a[2]:
            err = (a[2][k] - b[2][k]).norm().item()
            assert err <= 1e-5 * a[2][k].norm().item() + 1e-7, (k, err)
    finally:
        model.set_last_cls(None)


@pytest.mark.parametrize("ckpt", [False, True])
def test_backward_twice_over_one_forward(ckpt):
    """The second backward re-reads (kept activations) or re-forwards (recompute plan) the CLS-only block: the same gradients again."""
    spec, sd, x, meta = _case("two", 3)
    model = _model(spec, sd, "fp32")
    model.set_last_cls(True)
    try:
        model.train(True)
        model._inject_drop = _inject(spec, 3, "sample0")
        before = model.last_cls_blocks()
        out = model(x.cuda(), meta.cuda(), force_checkpointing=True) if ckpt else model(x.cuda(), meta.cuda())
        loss = O.probe_loss(out)
        loss.backward(retain_graph=True)
        g1 = _grads(model)
        model.zero_grad(set_to_none=True)
        loss.backward()
        g2 = _grads(model)
        assert model.last_cls_blocks() - before >= 1
        for k in g1:
            err = (g1[k] - g2[k]).norm().item()
            assert err <= 1e-5 * g1[k].norm().item() + 1e-7, (k, err)
    finally:
        model.set_last_cls(None)


def test_segment_wise_backward():
    """lnx_plan_backward segment by segment (what DataParallel's hook drives) against the one-call backward."""
    spec, sd, x, meta = _case("two", 3)
    model = _model(spec, sd, "fp32")
    xs, ms = x.cuda(), meta.cuda()
    inj = _inject(spec, 3, "sample0")
    try:
        a = _step(model, xs, ms, inj, True)
        seen = []
        model._segment_hook = seen.append
        b = _step(model, xs, ms, inj, True)
        assert seen == [0, 1, 2, 3] and b[3] == 1
        for k in a[2]:
            err = (a[2][k] - b[2][k]).norm().item()
            assert err <= 1e-5 * a[2][k].norm().item() + 1e-7, (k, err)
    finally:
        model._segment_hook = None
        model.set_last_cls(None)


def test_gradnorm_per_task_backwards():
    """One forward, one lnx_plan_backward_into per task: on against off."""
    spec, sd, x, meta = _case("two", 3)
    model = _model(spec, sd, "fp32")
    xs, ms = x.cuda(), meta.cuda()
    model.train(True)
    model._inject_drop = _inject(spec, 3, "sample0")
    O.probe_loss(model(xs, ms)).backward()  # binds the gradient arena
    T = len(spec.heads)

    def seeds(t, logits_t, dl_t):
        dl_t.copy_(torch.tanh(logits_t) * 0.01)

    res = {}
    try:
        for on in (False, True):
            model.set_last_cls(on)
            before = model.last_cls_blocks()
            res[on] = model._task_backbone_grads(xs, ms, seeds, n_arenas=T).clone()
            assert model.last_cls_blocks() - before == (1 if on else 0)
    finally:
        model.set_last_cls(None)
    for t in range(T):  # (the bound of test_gradnorm_forward_on_compact_rows)
        err = (res[True][t] - res[False][t]).norm().item()
        assert err <= 1e-5 * res[False][t].norm().item() + 1e-7, (t, err)


@pytest.mark.parametrize("cut", ["stages.3.1", "tail", "stages.3.0"])
def test_finetune_cut_at_the_last_block_and_around_it(cut):
    """The last block as the cut itself (its input gradient feeds nobody), behind the cut (forward only) and with the block before it
    trained too: the trained parameters' gradients on against off, the frozen ones get none."""
    spec, sd, x, meta = _case("two", 3)
    model = _model(spec, sd, "fp32")
    model.freeze_through(cut)
    xs, ms = x.cuda(), meta.cuda()
    inj = _inject(spec, 3, "sample0")
    res = {}
    try:
        for on in (False, True):
            model.set_last_cls(on)
            model.zero_grad(set_to_none=True)
            model.train(True)
            model._inject_drop = inj
            before = model.last_cls_blocks()
            out = model(xs, ms)
            O.probe_loss(out).backward()
            assert model.last_cls_blocks() - before == (1 if on else 0)
            res[on] = ({t: v.detach().clone() for t, v in out.items()}, {k: (None if p_.grad is None else p_.grad.detach().clone()) for k, p_ in model.named_parameters()})
    finally:
        model.set_last_cls(None)
    for t in res[True][0]:
        torch.testing.assert_close(res[True][0][t], res[False][0][t], rtol=1e-4, atol=1e-4)
    trained = 0
    for k, g in res[True][1].items():
        assert (g is None) == (res[False][1][k] is None), k
        if g is not None:
            trained += 1
            ref = res[False][1][k]
            assert (g - ref).norm().item() <= 2e-3 * max(ref.norm().item(), 1e-3), k  # test_backward_matches_oracle's fp32 bound
    assert trained > 0


def test_inference_plan_under_no_grad():
    spec, sd, x, meta = _case("two", 3)
    model = _model(spec, sd, "fp32")
    xs, ms = x.cuda(), meta.cuda()
    try:
        model.set_last_cls(True)
        model.train(False)
        model._inject_drop = None
        before = model.last_cls_blocks()
        with torch.no_grad():
            inf = {t: v.clone() for t, v in model(xs, ms).items()}
        assert model.last_cls_blocks() - before == 1
        n = O.n_drop_calls(spec)
        model.train(True)
        model._inject_drop = [None] * n  # a training plan without DropPath multipliers
        trn = model(xs, ms)
        ref = O.forward(sd, spec, x, meta)
        for t in inf:
            torch.testing.assert_close(inf[t], trn[t].detach(), rtol=1e-4, atol=1e-4)
            scale = max(1.0, ref[t].abs().max().item())
            torch.testing.assert_close(inf[t].cpu(), ref[t], rtol=1e-4, atol=1e-4 * scale)
    finally:
        model.set_last_cls(None)


def test_fp8_plan_keeps_the_full_block():
    spec = O.Spec(heads=(("taxa_L10", 10), ("taxa_L20", 5)), drop_path_rate=0.2)
    B = 8
    sd = O.seeded_state_dict(O.param_shapes(spec), 777)
    x, meta = O.seeded_inputs(spec, B, 224, 778)
    inj = _drop_scales(spec, B, 779)
    model = _model(spec, sd, "fp8", img=224)
    model.set_last_cls(True)
    try:
        before = model.last_cls_blocks()
        model.train(True)
        model._inject_drop = inj
        O.probe_loss(model(x.cuda(), meta.cuda())).backward()
        assert model.last_cls_blocks() == before
        assert all(torch.isfinite(p_.grad).all() for p_ in model.parameters())
        model.set_compute_dtype("bf16")
        model._inject_drop = inj
        O.probe_loss(model(x.cuda(), meta.cuda())).backward()
        assert model.last_cls_blocks() == before + 1
    finally:
        model.set_last_cls(None)


def test_drop_rate_plan_keeps_the_full_block():
    spec, sd, x, meta = _case("one", 3)
    model = _model(spec, sd, "fp32", DROP_RATE=0.2)
    model.set_last_cls(True)
    try:
        before = model.last_cls_blocks()
        model.train(True)
        model._inject_drop = _inject(spec, 3, "sample0")
        O.probe_loss(model(x.cuda(), meta.cuda())).backward()
        assert model.last_cls_blocks() == before
        assert all(torch.isfinite(p_.grad).all() for p_ in model.parameters())
    finally:
        model.set_last_cls(None)


if __name__ == "__main__":
    measure_off_against_off()
