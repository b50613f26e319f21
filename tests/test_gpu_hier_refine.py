"""The hierarchical refinement on the GPU (lnx_hier_refine_fwd / lnx_hier_refine_bwd behind linnaeus_amd.ops.hier_refine_fwd / _bwd,
linnaeus_amd.heads.HierarchicalRefinement and mFormerV1.forward) against the fp64 restatement tests/hier_refine_ref.py.

Tolerances.  fp32 forward: rtol = atol = 1e-5 against fp64 (the bound tests/test_gpu_model.py::test_opt_in_hierarchical_refinement sets
for this formula).  bf16: within one bf16 ulp of the expected value plus 1e-5, the expected value being the restatement with bf16
storage of ONE level fed with the parent row the kernel itself stored -- two fp32 / fp64 results a rounding error apart may land on
neighbouring bf16 numbers, and a parent row that differs by a bf16 ulp (6 % of a logit of 8) moves every child by more than an ulp, so
a chained comparison would test the luck of the draw.  fp32 gradients: against the restatement's fp64 backward, within TWICE the
largest error the fp32 torch composition (refine_logits_top_down and .backward()) makes on the same inputs against the same fp64
values (the summation orders differ); measured on an MI355X, largest |error| over all levels, kernel / torch composition:
    chain8 1.5e-05 / 3.9e-05    small 6.9e-08 / 2.9e-07    wide 1.0e-05 / 1.6e-05    gaps 1.1e-06 / 7.6e-06    deep 7.5e-07 / 7.7e-07
    gumbel 2.2e-05 / 1.5e-05
(with the segment sums carried in fp32 instead of fp64 the kernel was 2.9e-05 off in `gaps`, whose crowded parent owns 290 children).
bf16 gradients: one level at a time from the kernel's own stored G of the level below, one bf16 ulp plus 1e-5."""
import math
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn as nn

from linnaeus_amd import _lib as L
from linnaeus_amd import heads as H
from linnaeus_amd import ops
from tests import hier_refine_ref as R

pytestmark = pytest.mark.gpu

THREADS = 256  # HR_THREADS of csrc/hier_refine.hip: one workgroup per row, rows walked in strides of it
NAN = float("nan")

# name -> (class counts finest first, B, levels without a table, temperatures).  Class counts either side of the wave (64) and of the
# workgroup (256), 1 and 2, 1000 and 4099 (more than sixteen strides, as a child and as a parent level); B = 1, 3 and 300 (more rows than
# the chip has compute units);
# 1, 2, 4 and 8 levels.  Every case has orphans (parent = -1) at its finest level and parents without children.
CASES = {
    "chain8": ((4099, 1000, 257, 256, 255, 65, 64, 63), 3, (), (1.0, 0.7, 1.0, 1.3, 1.0, 1.0, 2.0, 1.0)),
    "small": ((64, 2, 1, 1), 1, (), (1.0, 0.5, 1.0, 1.0)),
    "wide": ((1000, 300), 300, (), (0.8, 1.0)),
    "gaps": ((400, 40, 12, 5), 3, (1,), (1.0, 1.0, 1.5, 1.0)),  # a level with no table between two that have one
    "single": ((257,), 3, (), (1.0,)),  # a pure pass-through
    "deep": ((5000, 4099), 3, (), (1.0, 1.0)),  # a PARENT level beyond the sixteen strides the backward keeps in registers
}


def bf16_ulp(x):
    """the spacing of bf16 numbers at |x| (8 significant bits), for fp64 x"""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -126)))
    return torch.exp2(e - 7)


def make_case(name, dtype, seed=7):
    Cs, B, gaps, temps = CASES[name]
    T = len(Cs)
    g = torch.Generator().manual_seed(seed + T)
    parents = []
    for t in range(T - 1):
        if t in gaps:
            parents.append(None)
            continue
        crowd = (3, THREADS + 74) if name == "gaps" and t == 0 else None  # one parent owns more children than the workgroup has threads
        barren = (1,) if Cs[t + 1] > 2 else ()
        parents.append(R.random_parents(Cs[t], Cs[t + 1], g, orphan_every=7 if t == 0 else 0, barren=barren, crowd=crowd))
    parents.append(None)
    if name == "gaps":
        assert int((parents[0] == 3).sum()) > THREADS
    bases = [(torch.randn(B, c, generator=g) * 2).to(dtype) for c in Cs]
    douts = [torch.randn(B, c, generator=g).to(dtype) for c in Cs]
    tables = []
    for t in range(T):
        if parents[t] is None:
            tables.append(None)
        else:
            start, idx = H.children_csr(parents[t], Cs[t + 1])
            tables.append((parents[t].cuda(), start.cuda(), idx.cuda()))
    return NS(name=name, Cs=Cs, B=B, T=T, parents=parents, tables=tables, bases=bases, douts=douts, temps=list(temps), modes=[L.HIER_ROUTE_SOFT] * T,
              noises=[None] * T, dtype=dtype)


def padded(x, pad=5):
    """x as a [:, :C] view of NaN-filled [B, C + pad] storage on the device -> (view, storage)"""
    store = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=x.dtype, device="cuda")
    view = store[:, : x.shape[1]]
    view.copy_(x)
    return view, store


def nan_like(x, pad=5):
    store = torch.full((x.shape[0], x.shape[1] + pad), NAN, dtype=x.dtype, device="cuda")
    return store[:, : x.shape[1]], store


def run_kernels(c, douts="all", pad=5):
    """forward and backward through the two launches, every tensor a padded view of NaN-filled storage"""
    bases = [padded(b, pad) for b in c.bases]
    outs = [nan_like(b, pad) for b in c.bases[:-1]] + [bases[-1]]  # the coarsest level: out is its base
    noises = [None if n is None else n.cuda() for n in c.noises]
    got, stats = ops.hier_refine_fwd([v for v, _ in bases], c.tables, c.modes, c.temps, noises, outs=[v for v, _ in outs])
    dts = [None if (douts != "all" and t in douts) else padded(d, pad) for t, d in enumerate(c.douts)]
    dbs = [nan_like(b, pad) for b in c.bases]
    dbases = ops.hier_refine_bwd(got, stats, [None if d is None else d[0] for d in dts], c.tables, c.modes, c.temps, noises, dbases=[v for v, _ in dbs])
    torch.cuda.synchronize()
    for t, ((_, bs), (_, os_), (_, ds)) in enumerate(zip(bases, outs, dbs)):
        C_ = c.Cs[t]
        for what, s in (("base", bs), ("out", os_), ("dbase", ds)):
            assert torch.isnan(s[:, C_:]).all(), f"level {t}: the {what} padding was written"
            assert not torch.isnan(s[:, :C_]).any(), f"level {t}: {what} holds a NaN inside C (not fully written)"
    return NS(outs=[o.clone() for o in got], dbases=[d.clone() for d in dbases], stats=stats)


def torch_composition(c):
    """refine_logits_top_down in fp32 on the case's inputs with .backward() of sum_t (out_t * dout_t).sum() -> (outs, grads)"""
    keys = [f"t_L{10 * (i + 1)}" for i in range(c.T)]
    heads = nn.ModuleDict()
    for t in range(c.T):
        m = nn.Module()
        m.temperature = c.temps[t]
        if c.parents[t] is not None:
            M = torch.zeros(c.Cs[t + 1], c.Cs[t])
            has = c.parents[t] >= 0
            M[c.parents[t][has].long(), torch.nonzero(has).reshape(-1)] = 1.0
            m.register_buffer(f"hmatrix_{keys[t + 1]}_{keys[t]}", M)
        heads[keys[t]] = m
    heads = heads.cuda()
    leaves = {k: b.float().cuda().requires_grad_(True) for k, b in zip(keys, c.bases)}
    out = H.refine_logits_top_down(leaves, heads, keys)
    sum((out[k] * d.float().cuda()).sum() for k, d in zip(keys, c.douts)).backward()
    return [out[k].detach().cpu() for k in keys], [leaves[k].grad.cpu() for k in keys]


def level_expected(c, t, parent_row, storage):
    """level t of the forward alone, from the given (stored) parent row"""
    if t == c.T - 1 or c.parents[t] is None:
        return c.bases[t].double()
    two = R.forward([c.bases[t], parent_row], [c.parents[t], None], [c.modes[t], 0], [c.temps[t], 1.0], [c.noises[t], None], storage)
    return two[0]


def check_forward(c, got):
    outs = [o.cpu() for o in got.outs]
    if c.dtype == torch.float32:
        want = R.forward(c.bases, c.parents, c.modes, c.temps, c.noises)
        for t in range(c.T):
            err = (outs[t].double() - want[t]).abs().max().item()
            print(f"{c.name} fp32 forward level {t} (C={c.Cs[t]}): max |error| {err:.3g}")
            torch.testing.assert_close(outs[t].double(), want[t], rtol=1e-5, atol=1e-5)
    else:
        for t in range(c.T):
            want = level_expected(c, t, outs[t + 1] if t + 1 < c.T else None, torch.bfloat16)
            over = ((outs[t].double() - want).abs() - bf16_ulp(want) - 1e-5).max().item()
            print(f"{c.name} bf16 forward level {t} (C={c.Cs[t]}): max (|error| - ulp - 1e-5) {over:.3g}")
            assert over <= 0, (t, over)
    for t in range(c.T):  # pass-through levels are copies
        if t == c.T - 1 or c.parents[t] is None:
            assert torch.equal(outs[t], c.bases[t]), t


def check_backward(c, got, bound=None, douts="all"):
    outs = [o.cpu() for o in got.outs]
    dbs = [d.cpu() for d in got.dbases]
    dts = [None if (douts != "all" and t in douts) else d for t, d in enumerate(c.douts)]
    if c.dtype == torch.float32:
        want = R.backward([o.double() for o in outs], dts, c.parents, c.modes, c.temps, c.noises)
        err = max((dbs[t].double() - want[t]).abs().max().item() for t in range(c.T))
        print(f"{c.name} fp32 backward: max |error| of the kernel {err:.3g}, allowed (twice the torch composition's) {bound:.3g}")
        assert err <= bound, (err, bound)
    else:
        for t in range(c.T):  # one level at a time: G of the level below as the kernel stored it
            want = _one_level_backward(c, t, outs, dbs[t - 1].double() if t > 0 else None, dts[t])
            over = ((dbs[t].double() - want).abs() - bf16_ulp(want) - 1e-5).max().item()
            print(f"{c.name} bf16 backward level {t}: max (|error| - ulp - 1e-5) {over:.3g}")
            assert over <= 0, (t, over)


def _one_level_backward(c, t, outs, G_below, dout):
    """G of level t from the stored G of level t - 1 (restatement, bf16 storage)"""
    g = torch.zeros_like(outs[t].double()) if dout is None else dout.double().clone()
    if t > 0 and c.parents[t - 1] is not None and c.modes[t - 1] != L.HIER_ROUTE_HARD:
        parent = c.parents[t - 1].long()
        has = parent.ge(0)
        S = torch.zeros_like(g).index_add_(1, parent[has], G_below[:, has])
        prob = R.routing_probs(outs[t].double(), c.modes[t - 1], c.temps[t - 1], c.noises[t - 1])
        dprob = S / (prob + R.EPS)
        g = g + prob * (dprob - (prob * dprob).sum(1, keepdim=True)) / c.temps[t - 1]
    return g.to(torch.bfloat16).double()


def gradient_bound(c32, fed=None):
    """twice the largest error of the fp32 torch composition against fp64 on the case's inputs (`fed`: the case the composition is
    given where it cannot take c32 itself)"""
    want_out = R.forward(c32.bases, c32.parents, c32.modes, c32.temps, c32.noises)
    want = R.backward(want_out, c32.douts, c32.parents, c32.modes, c32.temps, c32.noises)
    _, grads = torch_composition(fed or c32)
    err = max((grads[t].double() - want[t]).abs().max().item() for t in range(c32.T))
    print(f"{c32.name}: fp32 torch composition, max gradient |error| against fp64 {err:.3g}")
    return 2.0 * err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_kernels_match_the_restatement(name, dtype):
    """Both launches at every seam of CASES: values, NaN-filled padding (ld > C) that comes back untouched, NaN-filled out / dbase
    fully overwritten inside C."""
    c = make_case(name, dtype)
    got = run_kernels(c)
    check_forward(c, got)
    bound = gradient_bound(c) if dtype == torch.float32 and c.T > 1 else 0.0
    if c.T == 1:
        assert torch.equal(got.dbases[0].cpu(), c.douts[0])  # a pure pass-through
        return
    check_backward(c, got, bound)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_same_inputs_give_the_same_bits_and_null_dout_is_zeros(dtype):
    """No deterministic mode set: two runs are torch.equal in outputs and gradients (no atomics anywhere), and a NULL dout for some
    tasks gives what zeros give."""
    assert not L.is_deterministic()
    c = make_case("chain8", dtype)
    a, b = run_kernels(c), run_kernels(c)
    for t in range(c.T):
        assert torch.equal(a.outs[t], b.outs[t]) and torch.equal(a.dbases[t], b.dbases[t]), t
    assert torch.equal(a.stats, b.stats)
    none = run_kernels(c, douts=(0, 3, 7))
    for t in (0, 3, 7):
        c.douts[t] = torch.zeros_like(c.douts[t])
    zeros = run_kernels(c)
    for t in range(c.T):
        assert torch.equal(none.dbases[t], zeros.dbases[t]), t
    assert not torch.equal(none.dbases[1], a.dbases[1])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_hard_routing(dtype):
    """'hard' (eval): the children of the arg-max parent come back as their base, bit for bit; all others base + log(1e-10); nothing is
    sent up, so the parent level's dbase is its dout exactly; a tie takes the lowest index."""
    c = make_case("gaps", dtype)
    c.modes[0] = L.HIER_ROUTE_HARD  # level 0 routed from level 1 (40 classes)
    top = c.bases[1].max().item() + 1.0
    c.bases[1][0, 17] = c.bases[1][0, 5] = top  # row 0: a tie -> 5
    c.bases[1][1, 39] = top                      # row 1: the last class
    c.bases[1][2, 3] = top                       # row 2: the parent that owns more children than the workgroup has threads
    got = run_kernels(c)
    out0, base0 = got.outs[0].cpu(), c.bases[0]
    arg = torch.tensor([5, 39, 3])
    assert torch.equal(arg, c.bases[1].float().argmax(1))
    chosen = c.parents[0].long().unsqueeze(0) == arg.unsqueeze(1)  # [B, C0]
    assert chosen[2].sum() > THREADS
    assert torch.equal(out0[chosen], base0[chosen])
    want = base0.double() + math.log(1e-10)
    if dtype == torch.float32:
        torch.testing.assert_close(out0.double()[~chosen], want[~chosen], rtol=1e-5, atol=1e-5)
    else:
        assert (((out0.double() - want).abs() - bf16_ulp(want) - 1e-5)[~chosen] <= 0).all()
    assert torch.equal(got.dbases[1].cpu(), c.douts[1]) and torch.equal(got.dbases[0].cpu(), c.douts[0])
    # the levels above are routed softly as before
    soft = make_case("gaps", dtype)
    soft.bases[1] = c.bases[1]
    ref = run_kernels(soft)
    for t in (1, 2, 3):
        assert torch.equal(ref.outs[t], got.outs[t])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_gumbel_routing_with_replayed_noise(dtype):
    """'gumbel' (training) with given noise against the restatement; the gradient bound comes from the torch composition fed with
    base + noise (added in fp32, as F.gumbel_softmax adds it) at the pass-through parent level -- the same function -- against the
    fp64 values of the true inputs."""
    c = make_case("wide", dtype)
    g = torch.Generator().manual_seed(11)
    c.modes[0] = L.HIER_ROUTE_GUMBEL
    c.noises[0] = -torch.empty(c.B, c.Cs[1]).exponential_(generator=g).log()
    got = run_kernels(c)
    check_forward(c, got)
    bound = None
    if dtype == torch.float32:
        fed = make_case("wide", dtype)
        fed.bases[1] = c.bases[1] + c.noises[0]
        c.name = "gumbel"
        bound = gradient_bound(c, fed)
    check_backward(c, got, bound)
    soft = make_case("wide", dtype)
    assert not torch.equal(run_kernels(soft).outs[0], got.outs[0])  # the noise does route differently


# ---------------------------------------------------------------------------------------------------- HierarchicalRefinement
class _Head(nn.Module):
    def __init__(self, strategy=None, temperature=1.0):
        super().__init__()
        self.temperature = temperature
        if strategy is not None:
            self.routing_strategy = strategy


def _refinement(c, strategy=None):
    keys = [f"t_L{10 * (i + 1)}" for i in range(c.T)]
    heads = nn.ModuleDict()
    for t in range(c.T):
        m = _Head(strategy, c.temps[t])
        if c.parents[t] is not None:
            M = torch.zeros(c.Cs[t + 1], c.Cs[t])
            has = c.parents[t] >= 0
            M[c.parents[t][has].long(), torch.nonzero(has).reshape(-1)] = 1.0
            m.register_buffer(f"hmatrix_{keys[t + 1]}_{keys[t]}", M)
        heads[keys[t]] = m
    return H.HierarchicalRefinement(heads.cuda(), keys), heads, keys


def test_refinement_object_one_launch_per_direction_and_gumbel_draws():
    c = make_case("gaps", torch.float32)
    ref, heads, keys = _refinement(c, "gumbel")
    heads.train()
    lib = L.lib()
    leaves = {k: b.cuda().requires_grad_(True) for k, b in zip(keys, c.bases)}
    n0 = lib.lnx_hier_refine_launches()
    torch.manual_seed(123)
    out = ref(leaves)
    assert lib.lnx_hier_refine_launches() == n0 + 1
    assert out[keys[-1]] is leaves[keys[-1]]  # the coarsest task's tensor is returned as it came
    sum((out[k] * d.cuda()).sum() for k, d in zip(keys, c.douts)).backward()
    assert lib.lnx_hier_refine_launches() == n0 + 2
    torch.manual_seed(123)
    again = ref({k: b.cuda() for k, b in zip(keys, c.bases)})
    for k in keys:
        assert torch.equal(out[k], again[k]), k  # the same torch seed: the same noise, the same bits
    torch.manual_seed(124)
    other = ref({k: b.cuda() for k, b in zip(keys, c.bases)})
    assert not torch.equal(out[keys[0]], other[keys[0]])
    # the noise is drawn as F.gumbel_softmax draws it, level by level (finest first), and noise= replays it
    torch.manual_seed(123)
    drawn = {keys[t]: -torch.empty(c.B, c.Cs[t + 1], device="cuda").exponential_().log() for t in range(c.T - 1) if c.parents[t] is not None}
    replay = ref({k: b.cuda() for k, b in zip(keys, c.bases)}, noise=drawn)
    for k in keys:
        assert torch.equal(out[k], replay[k]), k
    c.modes = [L.HIER_ROUTE_GUMBEL if p is not None else 0 for p in c.parents]
    c.noises = [drawn[keys[t]].cpu() if keys[t] in drawn else None for t in range(c.T)]
    direct = run_kernels(c)  # the two launches themselves on that noise: the same bits, and those against the restatement
    check_forward(c, direct)
    for t, k in enumerate(keys):
        assert torch.equal(out[k].detach(), direct.outs[t]) and torch.equal(leaves[k].grad, direct.dbases[t]), k
    heads.eval()  # gumbel only in training: soft routing now, and no noise is drawn
    state = torch.cuda.get_rng_state()
    soft = ref({k: b.cuda() for k, b in zip(keys, c.bases)})
    assert torch.equal(state, torch.cuda.get_rng_state())
    want = R.forward(c.bases, c.parents, None, c.temps)
    torch.testing.assert_close(soft[keys[0]].cpu().double(), want[0], rtol=1e-5, atol=1e-5)


# ---------------------------------------------------------------------------------------------------- model level
def _build_tiny_c(golden_dir, head_type="ConditionalClassifier"):
    from linnaeus_amd import build_model
    from tests.cases import TinyTree, load_case, make_config, model_state_dict_from_oracle

    spec, z, sd, x, meta, drops = load_case("tiny_c", golden_dir)
    ncls = {t: c for t, c in spec.heads}
    tree = TinyTree({"taxa_L10": {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2}, "taxa_L20": {0: 0, 1: 0, 2: 1}}, [t for t, _ in spec.heads], ncls)
    model = build_model(make_config(spec, 64, head_type), num_classes=ncls, taxonomy_tree=tree)
    model.load_state_dict(model_state_dict_from_oracle(model, sd), strict=True)
    model = model.cuda()
    model.set_compute_dtype("fp32")
    model.hierarchical_refinement = True
    return model, spec, x.cuda()


def test_model_device_path_agrees_with_the_torch_composition(golden_dir, monkeypatch):
    """tiny_c, fp32 plan, flag on: logits within the forward bound, every parameter gradient within the bound the project sets for
    two fp32 backwards of one model that differ in summation order (test_recompute_plan_equals_kept_activations: 1e-5 of the norm);
    one launch per forward and per backward."""
    from oracle import mformer_oracle as O

    model, spec, x = _build_tiny_c(golden_dir)
    model.train()
    lib = L.lib()
    res = {}
    for path in ("1", "0"):
        monkeypatch.setenv("LNX_HIER_REFINE", path)
        model.zero_grad(set_to_none=True)
        n0 = lib.lnx_hier_refine_launches()
        out = model(x, None)
        n1 = lib.lnx_hier_refine_launches()
        O.probe_loss(out).backward()
        n2 = lib.lnx_hier_refine_launches()
        assert (n1 - n0, n2 - n1) == ((1, 1) if path == "1" else (0, 0)), (path, n0, n1, n2)
        res[path] = ({k: v.detach().clone() for k, v in out.items()}, {k: p_.grad.detach().clone() for k, p_ in model.named_parameters()})
    keys = [t for t, _ in spec.heads]
    for k in keys:
        torch.testing.assert_close(res["1"][0][k], res["0"][0][k], rtol=1e-5, atol=1e-5)
    assert torch.equal(res["1"][0][keys[-1]], res["0"][0][keys[-1]])
    for k, ga in res["0"][1].items():
        err = (ga - res["1"][1][k]).norm().item()
        assert err <= 1e-5 * ga.norm().item() + 1e-7, (k, err, ga.norm().item())


def test_model_refined_logits_feed_the_fused_loss_the_predictor_and_autocast(golden_dir):
    from linnaeus_amd import DevicePredictor
    from linnaeus_amd.loss import FusedHierarchicalLoss, GradientWeighting

    model, spec, x = _build_tiny_c(golden_dir, "HierarchicalSoftmax")
    keys = [t for t, _ in spec.heads]
    cfg = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=False), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=True, VAL=False))))
    crit = {t: torch.nn.CrossEntropyLoss(reduction="none") for t in keys}
    gw = GradientWeighting(keys, cfg, "static", init_weights={t: 1.0 for t in keys}).cuda()
    fused = FusedHierarchicalLoss(keys, crit, gw, cfg)
    model.train()
    out = model(x, None)
    targets = {t: torch.arange(x.shape[0], device="cuda") % c for t, c in spec.heads}
    total, _, _ = fused(out, targets, NS(get_null_mask_prob=lambda step: 1.0), 0)
    total.backward()
    assert torch.isfinite(total) and all(p_.grad is not None and torch.isfinite(p_.grad).all() for p_ in model.parameters())
    pred = DevicePredictor(keys, dict(spec.heads), taxonomy_tree=model.head[keys[0]], top_k=2)
    got = pred.predict(model, x)
    assert got["ids"].shape == (x.shape[0], 3, 2) and (got["count"] >= 1).all()
    model.train()
    n0 = L.lib().lnx_hier_refine_launches()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out16 = model(x, None)
    assert L.lib().lnx_hier_refine_launches() == n0 + 1
    assert all(v.dtype == torch.bfloat16 for v in out16.values())
    sum(v.float().sum() for v in out16.values()).backward()
    for k in keys[:-1]:
        torch.testing.assert_close(out16[k].float(), out[k].detach(), rtol=2.0 ** -6, atol=2.0 ** -6)


def test_flag_off_takes_neither_path(golden_dir):
    model, spec, x = _build_tiny_c(golden_dir)
    model.hierarchical_refinement = False
    model.eval()
    n0 = L.lib().lnx_hier_refine_launches()
    with torch.no_grad():
        model(x, None)
    assert L.lib().lnx_hier_refine_launches() == n0 and getattr(model, "_hier_refine", None) is None
