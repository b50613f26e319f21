"""Fine-tuning plans on the GPU: a frozen prefix of the model runs forward-only and the backward stops at the first unit that
trains (include/lnx.h, "Fine-tuning: a frozen prefix").  Every cut is compared with the all-trainable plan of the same forward:
logits bit-equal, trainable gradients within the bound test_recompute_plan_equals_kept_activations uses for the same reason
(atomically ordered sums), frozen parameters without a gradient."""
import ctypes as C

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from oracle import mformer_oracle as O
from tests.cases import CASES, load_case, make_config, model_state_dict_from_oracle

pytestmark = pytest.mark.gpu
IMG = {"tiny_b": 96, "tiny_c": 64, "tiny_dp": 64}
_FULL = {}    # (case, dtype) -> (logits, gradients) of the all-trainable plan, computed once
_ORACLE = {}  # case -> oracle gradients


def build(name, golden_dir, dtype, grad_mode="autograd"):
    spec, z, sd, x, meta, drops = load_case(name, golden_dir)
    model = build_model(make_config(spec, IMG[name]), num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda().train()
    model.grad_mode = grad_mode
    model.set_compute_dtype(dtype)
    model._inject_drop = drops
    return model, x.cuda(), (meta.cuda() if meta is not None else None)


def step(model, x, meta, zero=True, **kw):
    if zero:
        model.zero_grad(set_to_none=True)
    out = model(x, meta, **kw)
    O.probe_loss(out).backward()
    return {t: v.detach().clone() for t, v in out.items()}, {k: (None if p_.grad is None else p_.grad.detach().clone()) for k, p_ in model.named_parameters()}


def full_plan(name, golden_dir, dtype):
    if (name, dtype) not in _FULL:
        model, x, meta = build(name, golden_dir, dtype)
        _FULL[(name, dtype)] = step(model, x, meta)
        model.release_plans()
    return _FULL[(name, dtype)]


def close(g, ref, scale=1.0):
    err = (g.double() - scale * ref.double()).norm().item()
    return err <= 1e-5 * scale * ref.double().norm().item() + 1e-7, err


def check_against_full(model, out, grads, full, tag):
    fout, fgrads = full
    for t in fout:
        assert torch.equal(out[t], fout[t]), (tag, t)
    for k, p_ in model.named_parameters():
        if p_.requires_grad:
            assert grads[k] is not None, (tag, k)
            ok, err = close(grads[k], fgrads[k])
            assert ok, (tag, k, err, fgrads[k].norm().item())
        else:
            assert grads[k] is None, (tag, k)


def queries(model):
    lib, h = L.lib(), model._active["handle"]
    return lib.lnx_plan_first_trained_unit(h), lib.lnx_plan_last_backward_units(h), lib.lnx_plan_num_units(h)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_every_cut_matches_the_full_plan(dtype, golden_dir):
    full = full_plan("tiny_dp", golden_dir, dtype)
    for mode in ("autograd", "direct"):
        model, x, meta = build("tiny_dp", golden_dir, dtype, mode)
        units = model.plan_units()["units"]
        assert len(units) == 14
        for u, name in enumerate(units):
            model.freeze_through(name)
            out, grads = step(model, x, meta)
            check_against_full(model, out, grads, full, (mode, name))
            assert queries(model) == (u, len(units) - u, len(units)), (mode, name)
        model.release_plans()


def oracle_grads(name, golden_dir):
    if name not in _ORACLE:
        spec, z, sd, x, meta, drops = load_case(name, golden_dir)
        osd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
        O.probe_loss(O.forward(osd, spec, x, meta, drops)).backward()
        _ORACLE[name] = {k: v.grad for k, v in osd.items()}
    return _ORACLE[name]


@pytest.mark.parametrize("cut", ["tokens_1", "stages.2.1", "heads"])
def test_cut_against_the_oracle_fp32(cut, golden_dir):
    ref = oracle_grads("tiny_dp", golden_dir)
    model, x, meta = build("tiny_dp", golden_dir, "fp32")
    model.freeze_through(cut)
    _, grads = step(model, x, meta)
    err = tot = 0.0
    n = 0
    for k, p_ in model.named_parameters():
        if p_.requires_grad:
            err += (grads[k].cpu().double() - ref[k].double()).pow(2).sum().item()
            tot += ref[k].double().pow(2).sum().item()
            n += 1
    glob = (err / tot) ** 0.5
    print(f"[tiny_dp fp32 cut {cut}] {n} trainable tensors, global relative gradient error vs oracle {glob:.2e}")
    assert n > 0 and glob <= 1e-3, (cut, glob)


NAN_BITS = 0x7FC00BAD


@pytest.mark.parametrize("cut", ["tokens_1", "mid", "heads"])
def test_nothing_below_the_cut_is_touched(cut, golden_dir):
    model, x, meta = build("tiny_dp", golden_dir, "bf16")
    model.freeze_through(cut)
    out = model(x, meta)
    st = model._active
    info = model.plan_units()
    u = info["units"].index(cut)
    base = model._grad_arena.data_ptr()
    offs = [(v.data_ptr() - base) // 4 for v in model._grad_views]
    row = torch.zeros(model._grad_arena.numel(), device="cuda", dtype=torch.float32)
    bits = row.view(torch.int32)
    below = [i for i, pu in enumerate(info["unit_of"]) if pu < u]
    assert below
    for i in below:
        bits[offs[i]: offs[i] + st["params"][i].numel()] = NAN_BITS
    dl = torch.zeros(max(st["logits_numel"], 1), device="cuda", dtype=torch.float32)
    with torch.no_grad():
        for v, t in zip(model._task_views(st, dl, x.shape[0]), st["tasks"]):
            v.copy_(torch.softmax(out[t].detach().float(), -1))
    ptrs = (C.c_void_p * st["n"])(*[row.data_ptr() + 4 * o for o in offs])
    L.check(L.lib().lnx_plan_backward_into(st["handle"], C.c_void_p(dl.data_ptr()), None, ptrs, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "lnx_plan_backward_into")
    torch.cuda.synchronize()
    for i in below:
        assert bool((bits[offs[i]: offs[i] + st["params"][i].numel()] == NAN_BITS).all()), (cut, st["names"][i])
    assert L.lib().lnx_plan_last_backward_units(st["handle"]) == len(info["units"]) - u
    heads = [i for i, nm in enumerate(st["names"]) if nm.startswith("head.") and nm.endswith("weight")]
    assert all(row[offs[i]: offs[i] + st["params"][i].numel()].abs().sum().item() > 0 for i in heads)
    for i in below:
        bits[offs[i]: offs[i] + st["params"][i].numel()] = 0
    assert bool(torch.isfinite(row).all())  # (everything outside the pre-filled slices)


def test_non_prefix_freezes(golden_dir):
    full = full_plan("tiny_dp", golden_dir, "fp32")
    model, x, meta = build("tiny_dp", golden_dir, "fp32")
    units = model.plan_units()["units"]
    # one block frozen in the middle while the stem trains: the cut stays the stem
    for k, p_ in model.named_parameters():
        p_.requires_grad_(not k.startswith("stages.2.0."))
    out, grads = step(model, x, meta)
    check_against_full(model, out, grads, full, "stages.2.0 frozen")
    assert units[queries(model)[0]] == "stem"
    # the stage-3 metadata heads and the classification heads only: the gradient crosses both stage-3 blocks and stops at tokens_1
    for k, p_ in model.named_parameters():
        p_.requires_grad_((k.startswith("meta_") and "_head_1." in k) or k.startswith("head."))
    out, grads = step(model, x, meta)
    check_against_full(model, out, grads, full, "meta heads 1 + heads")
    assert any(k.startswith("meta_") and grads[k] is not None and grads[k].abs().sum().item() > 0 for k in grads)
    assert units[queries(model)[0]] == "tokens_1" and queries(model)[1] == len(units) - units.index("tokens_1")
    for k, p_ in model.named_parameters():
        p_.requires_grad_(k == "cls_token_2")
    out, grads = step(model, x, meta)
    check_against_full(model, out, grads, full, "cls_token_2")
    assert units[queries(model)[0]] == "tokens_2"


@pytest.mark.parametrize("name,cut", [("tiny_b", "mid"), ("tiny_c", "tokens_1")])
def test_cut_on_other_architectures(name, cut, golden_dir):
    """tiny_b: only_last_cls (no cl_1_fc / aggregate) and three metadata components; tiny_c: no metadata (tokens_k = the CLS token)."""
    full = full_plan(name, golden_dir, "fp32")
    model, x, meta = build(name, golden_dir, "fp32")
    model.freeze_through(cut)
    out, grads = step(model, x, meta)
    check_against_full(model, out, grads, full, (name, cut))
    units = model.plan_units()["units"]
    assert queries(model)[:2] == (units.index(cut), len(units) - units.index(cut))


def test_recompute_with_a_cut(golden_dir):
    full = full_plan("tiny_dp", golden_dir, "fp32")
    model, x, meta = build("tiny_dp", golden_dir, "fp32")
    model.freeze_through("stages.2.1")
    out, grads = step(model, x, meta, force_checkpointing=True)
    assert any(k[-1] for k in model._plans), "no recompute plan was created"
    check_against_full(model, out, grads, full, "recompute")
    B = x.shape[0]
    assert model.workspace_bytes(B, 64, recompute=True) <= model.workspace_bytes(B, 64, recompute=False)


def test_plan_cache_with_freeze_states(golden_dir):
    model, x, meta = build("tiny_dp", golden_dir, "bf16")
    model.max_cached_plans = 2
    step(model, x, meta)
    first = model._active["handle"].value
    model.freeze_through("mid")
    step(model, x, meta)
    assert model._active["handle"].value != first and len(model._plans) == 2
    model.freeze_through("stem")
    step(model, x, meta)
    assert model._active["handle"].value == first and len(model._plans) == 2  # the all-trainable plan again: same handle
    out = model(x, meta)  # its forward ...
    model.freeze_through("heads")
    step(model, x, meta)  # a third state
    model.freeze_through("tokens_2")
    step(model, x, meta)  # ... and a fourth: the all-trainable plan is evicted
    assert len(model._plans) == 2
    with pytest.raises(L.LnxError, match="evicted"):
        O.probe_loss(out).backward()


def test_accumulation_in_direct_mode(golden_dir):
    full = full_plan("tiny_dp", golden_dir, "fp32")
    model, x, meta = build("tiny_dp", golden_dir, "fp32", "direct")
    model.freeze_through("tokens_1")
    step(model, x, meta)
    _, grads = step(model, x, meta, zero=False)
    for k, p_ in model.named_parameters():
        if p_.requires_grad:
            ok, err = close(grads[k], full[1][k], 2.0)
            assert ok, (k, err)
        else:
            assert p_.grad is None, k


def test_freezing_after_a_direct_mode_step_leaves_no_stale_grad(golden_dir):
    """A parameter trained in direct mode keeps .grad = its arena slice; frozen afterwards without zero_grad it must not keep that view
    (the fused launches of a trained unit may write the slice, and an optimizer steps on `grad is not None`)."""
    full = full_plan("tiny_dp", golden_dir, "fp32")
    model, x, meta = build("tiny_dp", golden_dir, "fp32", "direct")
    step(model, x, meta)
    # only stages.3.0's norm1 frozen: behind the cut (the stem), inside a unit whose launches cover it
    for k, p_ in model.named_parameters():
        p_.requires_grad_(not k.startswith("stages.3.0.norm1."))
    _, grads = step(model, x, meta, zero=False)
    for k, p_ in model.named_parameters():
        if p_.requires_grad:
            ok, err = close(grads[k], full[1][k], 2.0)
            assert ok, (k, err)
        else:
            assert p_.grad is None, k
    model.freeze_through("tokens_2")  # ... and a whole prefix, again without zero_grad
    _, grads = step(model, x, meta, zero=False)
    for k, p_ in model.named_parameters():
        if p_.requires_grad:
            ok, err = close(grads[k], full[1][k], 1.0 if k.startswith("stages.3.0.norm1.") else 3.0)  # (norm1 started afresh: it had no .grad)
            assert ok, (k, err)
        else:
            assert p_.grad is None, k


CANARY = 1 << 20


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_dropout_masks_with_a_cut_stay_inside_the_workspace(dtype, golden_dir):
    """MODEL.DROP_RATE > 0: the forward of EVERY RoPE block, frozen or not, sends its proj / fc2 product through the sD scratch.  Cuts
    behind `mid` (no stage-3 backward) and at `heads` (no RoPE backward at all) against the full plan with the same injected masks, on
    a workspace followed by a canary: logits bit-equal, trainable gradients within the bound, not one byte behind the workspace written."""
    spec, z, sd, x, meta, drops = load_case("tiny_dp", golden_dir)
    cfg = make_config(spec, 64)
    cfg.MODEL.DROP_RATE = 0.2
    model = build_model(cfg, num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda().train()
    model.set_compute_dtype(dtype)
    model._inject_drop = drops
    B, E = x.shape[0], 1 + len(spec.meta)
    gen = torch.Generator().manual_seed(11)
    bufs = []
    for s in range(2):
        N = ((64 // 16) >> s) ** 2 + E
        C_, hid = spec.rope_dims[s], int(spec.rope_dims[s] * spec.mlp_ratio[s])
        for _ in range(spec.rope_depths[s]):
            bufs += [(torch.rand(B * N * w, generator=gen) < 0.8).to(torch.uint8) for w in (C_, hid, C_)]
    model._inject_dropout = torch.cat(bufs)
    x, meta = x.cuda(), meta.cuda()
    full = step(model, x, meta)
    for cut in ("tokens_2", "heads"):
        model.freeze_through(cut)
        model(x, meta)  # creates and binds the plan of this cut
        st = model._active
        wsb = model.workspace_bytes(B, 64)  # (the planner's bytes + 256 of alignment slack: what the module allocates)
        assert st["ws"].numel() == wsb
        big = torch.full((wsb + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
        st["ws"], st["ptrs"] = big, None  # bound again, on this buffer, by the next forward
        out, grads = step(model, x, meta)
        assert model._active is st and st["ws"] is big
        check_against_full(model, out, grads, full, ("dropout", dtype, cut))
        torch.cuda.synchronize()
        assert bool((big[wsb:] == 0xA5).all()), (cut, "the plan wrote behind its workspace")


def test_segment_wise_backward(golden_dir):
    model, x, meta = build("tiny_dp", golden_dir, "fp32")
    model.freeze_through("stages.2.0")
    _, want = step(model, x, meta)
    units_one = queries(model)[1]
    seen = []
    model._segment_hook = seen.append
    _, got = step(model, x, meta)
    model._segment_hook = None
    assert seen == [0, 1, 2, 3]
    assert queries(model)[1] == units_one == 14 - model.plan_units()["units"].index("stages.2.0")
    for k, p_ in model.named_parameters():
        if p_.requires_grad:
            ok, err = close(got[k], want[k])
            assert ok, (k, err)
        else:
            assert got[k] is None, k


def test_gradnorm_backbone_grads_with_a_frozen_trunk(golden_dir):
    model, x, meta = build("tiny_dp", golden_dir, "fp32")
    T = len(CASES["tiny_dp"].heads)

    def seeds(t, logits_t, dl_t):
        dl_t.copy_(torch.softmax(logits_t.float(), -1))

    want = model._task_backbone_grads(x, meta, seeds, n_arenas=T).clone()
    model.freeze_through("tokens_1")
    info = model.plan_units()
    u = info["units"].index("tokens_1")
    base = model._grad_arena.data_ptr()
    offs = [(v.data_ptr() - base) // 4 for v in model._grad_views]
    rows = model._gradnorm_arenas(T)
    rows.zero_()
    bits = rows.view(torch.int32)
    for i, pu in enumerate(info["unit_of"]):
        if pu < u:
            bits[:, offs[i]: offs[i] + info["params"][i].numel()] = NAN_BITS
    got = model._task_backbone_grads(x, meta, seeds, n_arenas=T, accumulate=True)  # (accumulate: the rows keep what they hold)
    torch.cuda.synchronize()
    assert got.data_ptr() == rows.data_ptr()
    for i, pu in enumerate(info["unit_of"]):
        sl = slice(offs[i], offs[i] + info["params"][i].numel())
        if pu < u:
            assert bool((got.view(torch.int32)[:, sl] == NAN_BITS).all()), info["names"][i]
        else:
            for t in range(T):
                ok, err = close(got[t, sl], want[t, sl])
                assert ok, (info["names"][i], t, err)


def test_set_trainable_refusals(golden_dir):
    model, x, meta = build("tiny_dp", golden_dir, "bf16")
    lib = L.lib()
    lib.lnx_plan_workspace_bytes.restype = C.c_int64
    n = len(model.plan_units()["names"])
    model(x, meta)
    assert lib.lnx_plan_set_trainable(model._active["handle"], b"\x01" * n) != 0  # a bound plan
    assert "bound" in lib.lnx_last_error().decode()
    for train, mask, word in ((True, None, "NULL"), (True, bytes(n), "all zero"), (False, b"\x01" * n, "inference")):
        cfg = model._make_cfg(2, 64, 64, train, False)
        h = C.c_void_p()
        L.check(lib.lnx_plan_create(C.byref(cfg), C.byref(h)), "lnx_plan_create")
        try:
            before = lib.lnx_plan_workspace_bytes(h)
            assert lib.lnx_plan_set_trainable(h, mask) != 0
            assert word in lib.lnx_last_error().decode()
            if train:
                L.check(lib.lnx_plan_set_trainable(h, b"\x01" * n), "lnx_plan_set_trainable")
                assert lib.lnx_plan_workspace_bytes(h) == before
        finally:
            lib.lnx_plan_destroy(h)


def test_sm_production_dispatch_with_a_frozen_trunk():
    """mFormerV1_sm @224, batch 8, bf16, DropPath 0.2 with seeded draws: the conv trunk frozen against the full plan of the same forward."""
    spec = O.Spec(heads=(("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20)), drop_path_rate=0.2)
    B = 8
    sd = O.seeded_state_dict(O.param_shapes(spec), 777)
    x, meta = O.seeded_inputs(spec, B, 224, 778)
    g = torch.Generator().manual_seed(779)
    drops = [None if p_ == 0.0 else torch.floor((1.0 - p_) + torch.rand(B, generator=g)) / (1.0 - p_) for p_ in O.drop_call_probs(spec)]
    model = build_model(make_config(spec, 224), num_classes={t: c for t, c in spec.heads})
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda().train()
    model.set_compute_dtype("bf16")
    model._inject_drop = drops
    x, meta = x.cuda(), meta.cuda()
    full = step(model, x, meta)
    model.freeze_through("tokens_1")
    out, grads = step(model, x, meta)
    check_against_full(model, out, grads, full, "sm tokens_1")
    units = model.plan_units()["units"]
    assert queries(model)[:2] == (units.index("tokens_1"), len(units) - units.index("tokens_1"))
    assert model.workspace_bytes(B, 224) < model.workspace_bytes(B, 224, trainable=[k for k, _ in model.named_parameters()])
