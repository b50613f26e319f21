"""Deterministic mode (mFormerV1.set_deterministic) on whole training steps: the same parameters, inputs and DropPath draws give the
same bits -- logits, loss, every gradient, and the parameters after fused optimizer steps -- whichever streams the backward uses,
and the gradients agree with the default mode's to the tolerances tests/test_gpu_model.py holds the default mode to.

Configurations: tests/cases.py's tiny_b (metadata tokens, two blocks a stage) and tiny_dp (DropPath 0.5), tiny_a with
MODEL.DROP_RATE / ATTN_DROP_RATE > 0 ("tiny_drop": the keep masks of lnx_plan_set_dropout / lnx_plan_set_attn_dropout, drawn per
forward from the seed the caller sets), and mFormerV1_sm at 8 x 224 x 224, where every kernel runs many workgroups; bf16 and fp32
plans, the fp8 plan of sm, and recompute plans (forward(force_checkpointing=True)).  The loss is the fused multi-task cross entropy
(one launch, loss sum on the device) or FusedHierarchicalLoss (weighted_hierarchical_loss(fused=True): soft-label criteria, class
weights, null masking with injected draws)."""
from types import SimpleNamespace as NS

import pytest
import torch

import linnaeus_amd
from linnaeus_amd import build_model
from linnaeus_amd.config import ConfigNode
from linnaeus_amd.loss import GradientWeighting, TaxonomyAwareLabelSmoothingCE, multitask_cross_entropy, weighted_hierarchical_loss
from oracle import mformer_oracle as O
from tests.cases import CASES, SEED, make_config, model_state_dict_from_oracle

pytestmark = pytest.mark.gpu
IMG = {"tiny_b": 96, "tiny_dp": 64, "tiny_drop": 64, "sm": 224}
BATCH = {"tiny_b": 3, "tiny_dp": 4, "tiny_drop": 4, "sm": 8}
# (configuration, compute dtype, loss, recompute plan)
CONFIGS = [("tiny_b", "fp32", "ce", False), ("tiny_b", "bf16", "ce", False), ("tiny_dp", "fp32", "ce", False), ("tiny_dp", "bf16", "ce", False),
           ("tiny_drop", "fp32", "ce", False), ("tiny_drop", "bf16", "ce", False), ("tiny_b", "bf16", "hier", False), ("tiny_dp", "fp32", "ce", True),
           ("sm", "fp32", "ce", False), ("sm", "bf16", "ce", False), ("sm", "fp8", "ce", False), ("sm", "bf16", "hier", False), ("sm", "bf16", "ce", True)]
HIER_CFG = NS(TRAIN=NS(PHASE1_MASK_NULL_LOSS=False), LOSS=NS(GRAD_WEIGHTING=NS(CLASS=NS(TRAIN=True, VAL=False))))


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    linnaeus_amd.set_deterministic(False)


def _drop_scales(spec, B, seed):
    """per-call, per-sample DropPath multipliers floor(keep + U) / keep, None where p == 0 (tests/test_gpu_model.py)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for p_ in O.drop_call_probs(spec):
        keep = 1.0 - p_
        out.append(None if p_ == 0.0 else torch.floor(keep + torch.rand(B, generator=g)) / keep)
    return out


class Case:
    def __init__(self, name, dtype, loss="ce", recompute=False):
        self.spec, self.B = CASES["tiny_a" if name == "tiny_drop" else name], BATCH[name]
        self.loss, self.recompute = loss, recompute
        self.sd = O.seeded_state_dict(O.param_shapes(self.spec), SEED)
        x, meta = O.seeded_inputs(self.spec, self.B, IMG[name], SEED + 1)
        self.x, self.meta = x.cuda(), (meta.cuda() if meta is not None else None)
        g = torch.Generator().manual_seed(SEED + 2)
        self.targets = {t: torch.randint(0, c, (self.B,), generator=g).cuda() for t, c in self.spec.heads}
        self.weights = {t: 1.0 / (i + 1) for i, (t, _) in enumerate(self.spec.heads)}
        cfg = make_config(self.spec, IMG[name])
        if name == "tiny_drop":
            cfg.MODEL.DROP_RATE, cfg.MODEL.ATTN_DROP_RATE = 0.1, 0.05
        self.model = build_model(cfg, num_classes={t: c for t, c in self.spec.heads}).cuda()
        self.model.set_compute_dtype(dtype)
        if loss == "hier":  # soft-label criteria, class weights, static task weights, null-masking draws (tests/test_gpu_hier_loss.py)
            self.crit, cw = {}, {}
            for t, c in self.spec.heads:
                self.targets[t][:max(1, self.B // 3)] = 0
                soft = 0.9 * torch.eye(c) + 0.1 * torch.softmax(torch.randn(c, c, generator=g), 1)
                self.crit[t] = TaxonomyAwareLabelSmoothingCE(soft / soft.sum(1, keepdim=True)).cuda()
                self.crit[t].validate_targets = False
                cw[t] = {i: float(0.5 + torch.rand(1, generator=g).item()) for i in range(0, c, 2)}
            self.coin = {t: torch.rand(self.B, generator=g).cuda() for t, _ in self.spec.heads}
            self.gw = GradientWeighting([t for t, _ in self.spec.heads], HIER_CFG, "static", init_weights=self.weights, class_weights=cw).cuda()
        self.reset()

    def reset(self):
        self.model.load_state_dict(model_state_dict_from_oracle(self.model, self.sd), strict=True)
        self.model.zero_grad(set_to_none=True)

    def step(self):
        """forward + fused loss + backward -> (logits, loss, gradients)"""
        m = self.model
        m.train(True)
        m._inject_drop = _drop_scales(self.spec, self.B, SEED + 3)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(SEED + 4)  # the dropout keep masks are drawn per forward from this
        out = m(self.x, self.meta, force_checkpointing=True) if self.recompute else m(self.x, self.meta)
        if self.loss == "hier":
            loss = weighted_hierarchical_loss(out, self.targets, self.crit, self.gw, NS(get_null_mask_prob=lambda step: 0.5), 0, config=HIER_CFG,
                                              sync_components=False, _coin=self.coin, fused=True)[0]
        else:
            loss = multitask_cross_entropy(out, self.targets, self.weights)
        loss.backward()
        torch.cuda.synchronize()
        return {t: v.detach().clone() for t, v in out.items()}, loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _same(a, b, what):
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), f"{what}: logits of {k} differ"
    assert torch.equal(a[1], b[1]), f"{what}: loss differs"
    diff = [k for k in a[2] if not torch.equal(a[2][k], b[2][k])]
    assert not diff, f"{what}: {len(diff)} of {len(a[2])} gradients differ, e.g. {diff[:6]}"


@pytest.mark.parametrize("name,dtype,loss,recompute", CONFIGS)
def test_training_step_is_bit_reproducible(name, dtype, loss, recompute):
    c = Case(name, dtype, loss, recompute)
    c.model.set_deterministic(True)
    assert linnaeus_amd.is_deterministic() and not c.model._plans
    first = c.step()
    for i in range(2):
        _same(first, c.step(), f"run {i + 2} against run 1")
    # whichever streams the backward uses: the weight-gradient stream, the metadata-head stream
    c.model.set_wgrad_stream(False)
    _same(first, c.step(), "weight-gradient stream off")
    c.model.set_wgrad_stream(True)
    for mode in (0, 2, 1):
        c.model.set_meta_stream(mode)
        _same(first, c.step(), f"meta stream mode {mode}")
    # the default mode computes the same gradients, to the bounds tests/test_gpu_model.py::test_backward_matches_oracle holds it to
    # against the oracle (per parameter 2e-3 fp32 / 10 % bf16, 25 % for the metadata-head chains; the whole gradient 1e-3 / 5 %), and
    # test_fp8_mode_sm_b24_against_oracle_and_bf16 the fp8 plans (the whole gradient 12 %, no bound per parameter)
    c.model.set_deterministic(False)
    off = c.step()
    fp32 = dtype == "fp32"
    tot_e = tot_r = 0.0
    for k, g in first[2].items():
        ref = off[2][k].double()
        err, den = (g.double() - ref).norm().item(), ref.norm().item()
        tot_e, tot_r = tot_e + err * err, tot_r + den * den
        tol = 2e-3 if fp32 else (0.25 if k.startswith("meta_") else 0.10)
        assert dtype == "fp8" or err <= tol * max(den, 1e-3 * (1 if fp32 else 10)), (k, err, den)
    assert (tot_e / tot_r) ** 0.5 <= {"fp32": 1e-3, "bf16": 5e-2, "fp8": 0.12}[dtype]


@pytest.mark.parametrize("name,dtype", [("tiny_b", "fp32"), ("tiny_b", "bf16"), ("tiny_drop", "bf16"), ("sm", "bf16")])
def test_optimizer_steps_are_bit_reproducible(name, dtype):
    """three AdamW steps of build_optimizer's configuration with the global clip, twice from the same start"""
    c = Case(name, dtype)
    c.model.set_deterministic(True)
    cfg = ConfigNode({"OPTIMIZER": {"NAME": "adamw"}, "TRAIN": {"CLIP_GRAD": 1.0}, "LR_SCHEDULER": {"BASE_LR": 1e-3}})
    ends = []
    for _ in range(2):
        c.reset()
        opt = linnaeus_amd.build_optimizer(cfg, c.model)
        for _ in range(3):
            c.step()
            opt.step()
        torch.cuda.synchronize()
        ends.append({k: p.detach().clone() for k, p in c.model.named_parameters()})
    start = model_state_dict_from_oracle(c.model, c.sd)
    assert any(not torch.equal(ends[0][k].cpu(), start[k]) for k in ends[0]), "the optimizer moved nothing"
    diff = [k for k in ends[0] if not torch.equal(ends[0][k], ends[1][k])]
    assert not diff, f"{len(diff)} of {len(ends[0])} parameters differ after three steps, e.g. {diff[:6]}"


def test_plan_created_outside_the_mode_refuses_to_run_in_it():
    c = Case("tiny_dp", "bf16")
    m = c.model
    m.train(True)
    m._inject_drop = _drop_scales(c.spec, c.B, SEED + 3)
    loss = multitask_cross_entropy(m(c.x, c.meta), c.targets, c.weights)
    linnaeus_amd.set_deterministic(True)  # the library's switch alone: the model's plans stay as they were created
    with pytest.raises(Exception, match="lnx_plan_backward: deterministic mode is on but this plan was created with it off"):
        loss.backward()
    torch.cuda.synchronize()
