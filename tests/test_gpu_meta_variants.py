"""Metadata variants from one trunk pass (lnx_plan_forward_tail, mFormerV1.forward_meta_variants) on the GPU.

The claim is bit equality: variant k of one forward_meta_variants call is what model(x, metas[k]) returns, because the tail re-runs the
same kernels on the same operands from the token boundary on.  Every comparison below is torch.equal; each case carries its control
(two plain forwards of the same input are torch.equal: the forward has no split-K and no atomic accumulation)."""
import ctypes as C
from collections import defaultdict
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model, collate
from linnaeus_amd.inference import DevicePredictor
from linnaeus_amd.metrics import DeviceMetrics, MetaVariantEvaluator
from oracle import mformer_oracle as O
from tests.cases import CASES, HEADS2, HEADS3, SEED, TINY_DIMS, TinyTree, make_config, model_state_dict_from_oracle

pytestmark = pytest.mark.gpu

IMG = 64
META3 = (("TEMPORAL", 2), ("SPATIAL", 3), ("ELEVATION", 10))
SPECS = {
    "tiny_b": CASES["tiny_b"],  # three components, only_last_cls, RoPE depths (2, 1)
    "tiny_a": CASES["tiny_a"],  # two components, the aggregation path (cl_1_fc, aggregate)
    # block outputs wrap around the ping-pong pair in both stages
    "deep": O.Spec(conv_dims=TINY_DIMS, conv_depths=(1, 1), rope_depths=(3, 2), rope_heads=(2, 4), meta=META3, heads=HEADS2),
    "hier": O.Spec(conv_dims=TINY_DIMS, conv_depths=(1, 1), rope_depths=(1, 1), rope_heads=(2, 4), meta=META3, heads=HEADS3),
    "nometa": CASES["tiny_c"],
}


@lru_cache(maxsize=None)
def _model(arch, dtype, rotate=False):
    spec = SPECS[arch]
    kw = {"num_classes": dict(spec.heads)}
    head_type = "Linear"
    if arch == "hier":
        head_type = "ConditionalClassifier"
        kw["taxonomy_tree"] = TinyTree({"taxa_L10": {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2}, "taxa_L20": {0: 0, 1: 0, 2: 1}}, [t for t, _ in spec.heads],
                                       dict(spec.heads))
    cfg = make_config(spec, IMG, head_type)
    if rotate:
        cfg.MODEL.ROPE_STAGES.ROPE_ROTATE = True
    model = build_model(cfg, **kw)
    sd = O.seeded_state_dict(O.param_shapes(spec), SEED)
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype(dtype)
    model.hierarchical_refinement = arch == "hier"
    return model.eval()


def _bounds(model):
    return {n: (i["offset"], i["offset"] + i["dim"]) for n, i in model.meta_components.items()}


def _combos(model):
    """unmasked, all zero, ["TEMPORAL"], ["SPATIAL", "ELEVATION"] (the components of the last that the model has)"""
    return [(), None, ["TEMPORAL"], [c for c in ("SPATIAL", "ELEVATION") if c in model.meta_components]]


def _inputs(model, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, IMG, IMG, generator=g).cuda()
    aux = torch.randn(B, sum(model.meta_dims), generator=g).cuda()
    return x, aux, collate.meta_variants(aux, _bounds(model), _combos(model))


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[t], b[t]) for t in a)


def _first_forward(model, x, m):
    """fp8: whether the plan takes these widths is the plan's own answer"""
    try:
        return model(x, m)
    except L.LnxError as e:
        if model.compute_dtype == "fp8" and "fp8" in str(e):
            pytest.skip(f"the plan refuses fp8 at the tiny widths: {e}")
        raise


CASES_EQ = [
    # arch, dtype, B, last_cls switch (None: the default), rotate
    ("tiny_b", "fp32", 1, None, False), ("tiny_b", "bf16", 3, None, False), ("tiny_b", "fp8", 3, None, False),
    ("tiny_a", "bf16", 1, None, False), ("tiny_a", "fp32", 3, None, False),
    ("deep", "bf16", 3, None, False), ("deep", "fp32", 1, None, False),
    ("tiny_b", "bf16", 3, True, False), ("tiny_b", "bf16", 3, False, False), ("deep", "fp32", 3, False, False),
    ("tiny_b", "bf16", 3, None, True),
    ("hier", "fp32", 3, None, False),
]


@pytest.mark.parametrize("arch,dtype,B,last_cls,rotate", CASES_EQ)
def test_variants_equal_plain_forwards_bit_for_bit(arch, dtype, B, last_cls, rotate):
    model = _model(arch, dtype, rotate)
    x, _, metas = _inputs(model, B)
    tasks = [t for t, _ in SPECS[arch].heads]
    model.set_last_cls(last_cls)
    try:
        with torch.no_grad():
            _first_forward(model, x, metas[0])
            before = model.last_cls_blocks()
            outs = model.forward_meta_variants(x, metas)
            ran_cls_only = model.last_cls_blocks() - before
            feats = model.forward_features_meta_variants(x, list(metas.unbind(0)))  # the other accepted form of `metas`
            assert len(outs) == len(feats) == 4
            for k in range(4):
                plain, again = model(x, metas[k]), model(x, metas[k])
                assert _same(plain, again), f"control: two plain forwards of variant {k} differ"
                assert sorted(outs[k]) == sorted(tasks) and _same(outs[k], plain), f"variant {k}"
                assert outs[k][tasks[0]].dtype == plain[tasks[0]].dtype
                assert torch.equal(feats[k], model.forward_features(x, metas[k])), f"features of variant {k}"
            # the variants are different computations, and nothing returned aliases anything else
            assert not torch.equal(outs[0][tasks[0]], outs[1][tasks[0]]) and not torch.equal(feats[0], feats[2])
            ptrs = [o[t].data_ptr() for o in outs for t in tasks] + [f.data_ptr() for f in feats]
            assert len(set(ptrs)) == len(ptrs)
        # the tails follow the forward's CLS-only decision: all four passes of the call, or none (fp8 plans keep the full block)
        expect_cls = (last_cls is not False) and dtype != "fp8"
        assert ran_cls_only == (4 if expect_cls else 0)
    finally:
        model.set_last_cls(None)


@pytest.mark.parametrize("arch,dtype", [("tiny_b", "bf16"), ("deep", "fp32")])
def test_the_tail_leaves_the_trunk_intact(arch, dtype):
    model = _model(arch, dtype)
    x, _, metas = _inputs(model, 3)
    m0, m1 = metas[0], metas[2]
    with torch.no_grad():
        r = model.forward_meta_variants(x, [m0, m1, m0, m1])
        assert _same(r[0], r[2]) and _same(r[1], r[3]) and not _same(r[0], r[1])
        fwd = model.forward_meta_variants(x, metas)
        rev = model.forward_meta_variants(x, metas.flip(0))
        for k in range(4):
            assert _same(fwd[k], rev[3 - k]), f"variant {k} depends on its place in the call"
        # a plain forward (of another batch, on the same plan) between two calls disturbs neither
        other = torch.randn_like(x)
        between = model(other, m1)
        again = model.forward_meta_variants(x, metas)
        assert all(_same(a, b) for a, b in zip(fwd, again)) and _same(between, model(other, m1))


def _raw_tail(st, meta, feats_ptr, logits_ptr):
    return L.lib().lnx_plan_forward_tail(st["handle"], C.c_void_p(meta.data_ptr()) if meta is not None else None, C.c_void_p(feats_ptr),
                                         C.c_void_p(logits_ptr), C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("arch,dtype", [("tiny_b", "bf16"), ("tiny_a", "fp32")])
def test_sentinels_every_exposed_element_is_written_and_nothing_else(arch, dtype):
    """Through the C ABI on the model's bound plan: per variant [guard | feats | guard | logits | guard] in one buffer, logits pre-filled
    with NaN, guards with a pattern; after each tail only that variant's feats / logits have changed."""
    model = _model(arch, dtype)
    B, G = 3, 64
    x, _, metas = _inputs(model, B)
    with torch.no_grad():
        plain = [model(x, m) for m in metas]
        plain_feats = [model.forward_features(x, m) for m in metas]
        model(x, metas[0])  # the trunk the tails below continue from
    st = model._active
    assert L.lib().lnx_plan_trunk_valid(st["handle"]) == 1
    nf, nl = B * model._dims[3], -(-st["logits_numel"] // 64) * 64
    per = G + nf + G + nl + G
    pattern = -12345.5
    buf = torch.full((3 * per,), pattern, device="cuda")
    slots = []
    for k in range(3):
        base = k * per
        f, lg = buf[base + G: base + G + nf], buf[base + 2 * G + nf: base + 2 * G + nf + nl]
        f.fill_(float("nan"))
        lg.fill_(float("nan"))
        slots.append((f, lg))
    torch.cuda.synchronize()
    for k, (f, lg) in enumerate(slots):
        snapshot = buf.clone()
        assert _raw_tail(st, metas[k + 1].contiguous(), f.data_ptr(), lg.data_ptr()) == 0, L.lib().lnx_last_error()
        torch.cuda.synchronize()
        changed = (buf != snapshot) & ~(buf.isnan() & snapshot.isnan())
        inside = torch.zeros_like(changed)
        base = k * per
        inside[base + G: base + G + nf] = True
        inside[base + 2 * G + nf: base + 2 * G + nf + nl] = True
        assert not (changed & ~inside).any(), f"tail {k + 1} wrote outside its own buffers"
        assert torch.equal(f.view(B, -1), plain_feats[k + 1])
        views = model._task_views(st, lg, B)
        for t, v in zip(st["tasks"], views):
            assert not v.isnan().any() and torch.equal(v, plain[k + 1][t].float()), (k, t)
    guards = torch.ones_like(buf, dtype=torch.bool)
    for k in range(3):
        base = k * per
        guards[base + G: base + G + nf] = False
        guards[base + 2 * G + nf: base + 2 * G + nf + nl] = False
    assert (buf[guards] == pattern).all()


def test_state_rules_on_the_device():
    lib = L.lib()
    model = _model("tiny_b", "bf16")
    x, _, metas = _inputs(model, 3)
    with torch.no_grad():
        ref = model(x, metas[1])
        model(x, metas[0])
    st = model._active
    feats = torch.empty(3, model._dims[3], device="cuda")
    logits = torch.empty(max(st["logits_numel"], 1), device="cuda")
    assert lib.lnx_plan_trunk_valid(st["handle"]) == 1
    # a failed call (NULL meta) discards the trunk; a fresh forward brings one back
    assert _raw_tail(st, None, feats.data_ptr(), logits.data_ptr()) != 0 and b"NULL" in lib.lnx_last_error()
    assert lib.lnx_plan_trunk_valid(st["handle"]) == 0
    assert _raw_tail(st, metas[1], feats.data_ptr(), logits.data_ptr()) != 0 and b"trunk" in lib.lnx_last_error()
    with torch.no_grad():
        model(x, metas[0])
    assert lib.lnx_plan_trunk_valid(st["handle"]) == 1
    assert _raw_tail(st, metas[1], feats.data_ptr(), logits.data_ptr()) == 0, lib.lnx_last_error()
    assert lib.lnx_plan_trunk_valid(st["handle"]) == 1
    for t, v in zip(st["tasks"], model._task_views(st, logits, 3)):
        assert torch.equal(v, ref[t].float())
    # lnx_plan_bind discards it as well
    torch.cuda.synchronize()
    st["ptrs"] = None
    model._ensure_bound(st)
    assert lib.lnx_plan_trunk_valid(st["handle"]) == 0
    assert _raw_tail(st, metas[1], feats.data_ptr(), logits.data_ptr()) != 0 and b"trunk" in lib.lnx_last_error()
    with torch.no_grad():  # and the model goes on as before
        assert _same(model(x, metas[1]), ref)
    # a training plan never holds a trunk
    model.train()
    try:
        model(x, metas[0])
        tr = model._active
        assert tr is not st and lib.lnx_plan_trunk_valid(tr["handle"]) == 0
        assert _raw_tail(tr, metas[1], feats.data_ptr(), logits.data_ptr()) != 0 and b"inference" in lib.lnx_last_error()
    finally:
        model.eval()
        model.release_plans()


def _nt_launches():
    return sum(L.lib().lnx_nt_kernel_launches(k) for k in range(16))


@pytest.mark.parametrize("arch,dtype", [("tiny_b", "bf16"), ("tiny_a", "fp32")])
def test_launch_accounting(arch, dtype):
    """K variants in one call issue (K - 1) x (NT launches of one forward's trunk) fewer NT launches than K plain forwards; the trunk's
    count is what a plain forward issues beyond a tail (the stem and downsample products, the conv blocks' where unfused)."""
    model = _model(arch, dtype)
    x, _, metas = _inputs(model, 3)
    K = 4
    with torch.no_grad():
        model(x, metas[0])  # (plan creation and binding are behind us)
        n0 = _nt_launches()
        model(x, metas[0])
        forward = _nt_launches() - n0
        st = model._active
        feats = torch.empty(3, model._dims[3], device="cuda")
        logits = torch.empty(max(st["logits_numel"], 1), device="cuda")
        n0 = _nt_launches()
        assert _raw_tail(st, metas[1], feats.data_ptr(), logits.data_ptr()) == 0, L.lib().lnx_last_error()
        tail = _nt_launches() - n0
        trunk = forward - tail
        assert tail > 0 and trunk >= 2  # at least the two downsample products in front of the token boundary
        n0 = _nt_launches()
        model.forward_meta_variants(x, metas)
        variants = _nt_launches() - n0
        n0 = _nt_launches()
        for k in range(K):
            model(x, metas[k])
        plain = _nt_launches() - n0
    assert plain == K * forward
    assert plain - variants == (K - 1) * trunk


def test_profile_spans_of_a_tail_are_the_rope_blocks_of_a_forward():
    """Under lnx_plan_profile_begin_spans a forward leaves one class-9 span per conv block and one class-8 span per RoPE block; a tail
    leaves the class-8 spans alone."""
    lib = L.lib()
    model = _model("deep", "bf16")
    x, _, metas = _inputs(model, 3)
    NC = 10

    def spans(fn):
        L.check(lib.lnx_plan_profile_begin_spans(st["handle"]), "lnx_plan_profile_begin_spans")
        fn()
        ms, work, byts, cnt = (C.c_double * NC)(), (C.c_double * NC)(), (C.c_double * NC)(), (C.c_int * NC)()
        L.check(lib.lnx_plan_profile_end_ex(st["handle"], ms, work, byts, cnt), "lnx_plan_profile_end_ex")
        return list(cnt), list(work)

    with torch.no_grad():
        model(x, metas[0])
        st = model._active
        feats = torch.empty(3, model._dims[3], device="cuda")
        logits = torch.empty(max(st["logits_numel"], 1), device="cuda")
        fwd_cnt, fwd_work = spans(lambda: model(x, metas[0]))
        tail_cnt, tail_work = spans(lambda: L.check(_raw_tail(st, metas[1], feats.data_ptr(), logits.data_ptr()), "lnx_plan_forward_tail"))
    assert fwd_cnt[8] == 5 and fwd_cnt[9] == 2  # RoPE depths (3, 2), conv depths (1, 1)
    assert tail_cnt[8] == 5 and tail_cnt[9] == 0 and tail_work[8] == fwd_work[8]
    assert sum(tail_cnt) == 5


def _targets(spec, B, seed):
    g = torch.Generator().manual_seed(seed)
    return {t: torch.randint(0, c, (B,), generator=g).cuda() for t, c in spec.heads}


def _ce(outputs, targets):
    return {t: torch.nn.functional.cross_entropy(outputs[t].float(), targets[t], reduction="none") for t in outputs}


def _tracker(phases):
    tr = SimpleNamespace()
    for name in ("chain_correct", "chain_total", "partial_chain_correct", "partial_chain_total"):
        setattr(tr, name, defaultdict(int))
    for name in ("partial_task_sums", "partial_null_sums", "partial_non_null_sums"):
        setattr(tr, name, {ph: defaultdict(lambda: defaultdict(float)) for ph in phases})
    for name in ("partial_task_counts", "partial_null_counts", "partial_non_null_counts"):
        setattr(tr, name, {ph: defaultdict(lambda: defaultdict(int)) for ph in phases})
    return tr


def _assert_metrics_equal(a, b, path=""):
    assert type(a) is type(b) or {type(a), type(b)} <= {int, float}, path
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            _assert_metrics_equal(a[k], b[k], f"{path}/{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (u, v) in enumerate(zip(a, b)):
            _assert_metrics_equal(u, v, f"{path}[{i}]")
    elif isinstance(a, int):
        assert a == b, path  # counters: exact
    else:
        # float64 sums of the same addends; their order inside a launch is the only freedom (2^-40 is far above it and far below any
        # real difference: one sample's loss is O(1) of a sum of twelve)
        assert a == pytest.approx(b, rel=2.0 ** -40, abs=0.0), path


def test_meta_variant_evaluator_equals_device_metrics_on_plain_forwards():
    spec = SPECS["tiny_b"]
    model = _model("tiny_b", "bf16")
    tasks, ncls = [t for t, _ in spec.heads], dict(spec.heads)
    combos = _combos(model)[:3]  # one phase name of each kind
    phases = collate.variant_phase_names(combos)
    assert phases == ["val", "val_mask_meta", "val_mask_TEMPORAL"]
    batches = [(*_inputs(model, 4, seed=70 + i)[:2], _targets(spec, 4, 80 + i)) for i in range(3)]
    ev = MetaVariantEvaluator(model, _bounds(model), combos, tasks, ncls, null_tracking_tasks=[tasks[0]], per_sample_loss=_ce)
    ref = {ph: DeviceMetrics(tasks, ncls, null_tracking_tasks=[tasks[0]]) for ph in phases}
    for x, aux, tg in batches:
        ev.update(x, aux, tg)
        with torch.no_grad():
            for ph, m in zip(phases, collate.meta_variants(aux, _bounds(model), combos)):
                out = model(x, m)
                ref[ph].update(out, tg, per_sample_losses=_ce(out, tg))
    got = ev.compute()
    assert list(got) == phases
    for ph in phases:
        want = ref[ph].compute()
        assert want["counts"]["tasks"][tasks[0]]["n"] == 12 and want["counts"]["tasks"][tasks[0]]["loss_n"] == 12
        _assert_metrics_equal(got[ph], want, ph)
    tr, tr_ref = _tracker(phases), _tracker(phases)
    ev.flush_into(tr)
    for ph in phases:
        ref[ph].flush_into(tr_ref, ph)
        assert tr.chain_total[ph] == tr_ref.chain_total[ph] == 12 and tr.chain_correct[ph] == tr_ref.chain_correct[ph]
        for t in tasks:
            assert dict(tr.partial_task_counts[ph][t]) == dict(tr_ref.partial_task_counts[ph][t]) == {"acc1": 12, "acc3": 12, "loss": 12}
            assert tr.partial_task_sums[ph][t]["acc1"] == tr_ref.partial_task_sums[ph][t]["acc1"]
            assert tr.partial_task_sums[ph][t]["loss"] == pytest.approx(tr_ref.partial_task_sums[ph][t]["loss"], rel=2.0 ** -40)
    assert ev.compute()["val"]["counts"]["chain_total"] == 0  # flushed means reset


def test_predict_variants_equals_predict_per_variant():
    spec = SPECS["tiny_b"]
    model = _model("tiny_b", "bf16")
    x, _, metas = _inputs(model, 3)
    tasks, ncls = [t for t, _ in spec.heads], dict(spec.heads)
    parents = {tasks[0]: torch.arange(ncls[tasks[0]]) % ncls[tasks[1]]}
    pred = DevicePredictor(tasks, ncls, parent_index=parents, top_k=3)
    got = pred.predict_variants(model, x, metas)
    assert len(got) == 4
    for k in range(4):
        want = pred.predict(model, x, metas[k])
        for name in ("ids", "probs", "count", "flags"):
            assert torch.equal(got[k][name], want[name]), (k, name)
    assert not torch.equal(got[0]["probs"], got[1]["probs"])


def test_refusals_of_the_model_call():
    model = _model("tiny_b", "bf16")
    x, _, metas = _inputs(model, 3)
    model.train()
    try:
        with pytest.raises(RuntimeError, match=r"torch\.no_grad\(\)"):
            model.forward_meta_variants(x, metas)
        with torch.no_grad():  # training mode without gradients takes an inference plan: allowed
            assert len(model.forward_meta_variants(x, metas)) == 4
    finally:
        model.eval()
    with torch.no_grad():
        with pytest.raises(ValueError):
            model.forward_meta_variants(x, metas[:, :, :-1])  # width
        with pytest.raises(ValueError):
            model.forward_meta_variants(x, metas[:, :2])  # batch
        with pytest.raises(ValueError):
            model.forward_meta_variants(x, [])
        with pytest.raises(ValueError):
            model.forward_meta_variants(x, metas[0])  # one [B, W] tensor is no list of variants
        nometa = _model("nometa", "fp32")
        with pytest.raises(ValueError, match="metadata"):
            nometa.forward_meta_variants(x, [torch.zeros(3, 5).cuda()])
        with pytest.raises(ValueError, match="metadata"):
            nometa.forward_features_meta_variants(x, [torch.zeros(3, 5).cuda()])


def test_meta_variants_masks_what_mask_meta_components_masks():
    model = _model("tiny_b", "bf16")
    bounds, combos = _bounds(model), _combos(model)
    aux = torch.randn(5, 15).cuda().abs() + 1.0  # (no zeros of its own)
    keep = aux.clone()
    mv = collate.meta_variants(aux, bounds, combos)
    assert mv.shape == (4, 5, 15) and mv.dtype == aux.dtype and torch.equal(aux, keep)
    assert torch.equal(mv[0], aux) and not mv[1].any()
    assert torch.equal(mv[2], collate.mask_meta_components(aux, bounds, ["TEMPORAL"])) and not mv[2][:, :2].any() and torch.equal(mv[2][:, 2:], aux[:, 2:])
    assert not mv[3][:, 2:].any() and torch.equal(mv[3][:, :2], aux[:, :2])
