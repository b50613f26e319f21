"""The configured optimizer on the host: `build_optimizer` against what the reference's optimizers/build.py builds on mFormerV1_sm
(tests/golden/optim_build.json, written by tests/golden/gen/make_golden_optim_build.py), the refusals, FusedSGD's constructor and
state-dict exchange with torch.optim.SGD, lnx_sgd_step's host validation, the ABI structs, and FusedMultiOptimizer's state dict.
The device path is in tests/test_gpu_optim_build.py."""
import ctypes as C
import json
import os
import shutil
import subprocess
import warnings

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import build_model
from linnaeus_amd.config import ConfigNode
from linnaeus_amd.optim import FusedAdamW, FusedAdEMAMix, FusedMultiOptimizer, FusedMuon, FusedSGD, build_optimizer
from tests.cases import CASES, make_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(REPO, "tests", "golden", "optim_build.json")))
CLASS_OF = {"SGD": FusedSGD, "AdamW": FusedAdamW, "AdEMAMix": FusedAdEMAMix, "Muon": FusedMuon}
KEYS = {"SGD": ("lr", "momentum", "dampening", "weight_decay", "nesterov"), "AdamW": ("lr", "betas", "eps", "weight_decay"),
        "AdEMAMix": ("lr", "betas", "eps", "weight_decay", "alpha", "T_alpha_beta3"), "Muon": ("lr", "weight_decay", "momentum", "nesterov", "ns_steps")}


@pytest.fixture(scope="module")
def sm():
    spec = CASES["sm"]
    model = build_model(make_config(spec, 224), num_classes={t: c for t, c in spec.heads})
    names = [n for n, _ in model.named_parameters()]
    assert names == GOLDEN["names"] and [p.dim() for p in model.parameters()] == GOLDEN["dims"]
    return model, {id(p): n for n, p in model.named_parameters()}


def cfg_for(rec, **train):
    cfg = ConfigNode({"OPTIMIZER": rec["overrides"], "LR_SCHEDULER": {"BASE_LR": rec["base_lr"]}, "TRAIN": {"CLIP_GRAD": rec["clip_grad"]}})
    cfg.TRAIN.merge(train)
    return cfg


def sub_optimizers(opt):
    return opt.optimizers if isinstance(opt, FusedMultiOptimizer) else {"": opt}


@pytest.mark.parametrize("cname", sorted(GOLDEN["configs"]))
def test_build_optimizer_reproduces_the_reference(sm, cname):
    model, name_of = sm
    rec = GOLDEN["configs"][cname]
    four_d = {n for n, d in zip(GOLDEN["names"], GOLDEN["dims"]) if d == 4}
    opt = build_optimizer(cfg_for(rec), model)
    assert (type(opt).__name__ == "FusedMultiOptimizer") == (rec["kind"] == "MultiOptimizer")
    subs = sub_optimizers(opt)
    assert list(subs) == list(rec["optimizers"])  # the same sub-optimizers, in the reference's insertion order
    muon_4d = set()
    for oname, want in rec["optimizers"].items():
        got = subs[oname]
        assert type(got) is CLASS_OF[want["class"]], (oname, type(got))
        assert len(got.param_groups) == len(want["groups"])
        for g, w in zip(got.param_groups, want["groups"]):
            names, wnames = [name_of[id(p)] for p in g["params"]], [GOLDEN["names"][i] for i in w["params"]]
            if want["ordered"]:
                assert names == wnames, (cname, oname)
            else:  # the reference iterates a Python set there: only the membership is defined
                assert sorted(names) == sorted(wnames), (cname, oname)
                order = {n: i for i, n in enumerate(GOLDEN["names"])}
                if want["class"] != "Muon":  # here: named_parameters() order (Muon: 2-D first, then 4-D, each in that order)
                    assert names == sorted(names, key=order.get)
            for k in KEYS[want["class"]]:
                a, b = g[k], w[k]
                assert (tuple(a) == tuple(b)) if isinstance(b, list) else (a == pytest.approx(b, rel=1e-12) if isinstance(b, float) else a == b), (cname, oname, k, a, b)
            if want["class"] == "Muon":
                muon_4d |= set(wnames) & four_d
    if rec["kind"] == "MultiOptimizer":
        assert [[g["optimizer_name"], g["optimizer_group_idx"]] for g in opt.param_groups] == rec["param_group_tags"]
        assert opt.max_grad_norm == rec["clip_grad"] and all(o.max_grad_norm is None for o in subs.values())
    else:
        assert opt.max_grad_norm == rec["clip_grad"]  # a single optimizer clips by itself
    # 4-D weights under Muon: trained here, left out of every optimizer with freeze_4d_like_reference
    frozen = build_optimizer(cfg_for(rec), model, freeze_4d_like_reference=True)
    held = {name_of[id(p)] for o in sub_optimizers(frozen).values() for g in o.param_groups for p in g["params"]}
    everything = {name_of[id(p)] for o in subs.values() for g in o.param_groups for p in g["params"]}
    assert everything == set(GOLDEN["names"])
    assert held == everything - muon_4d
    if cname in ("muon", "pg_muon"):
        assert muon_4d and muon_4d <= four_d
    else:
        assert not muon_4d


def test_clip_argument_and_config_defaults(sm):
    model, _ = sm
    opt = build_optimizer(ConfigNode({}), model)  # nothing configured: the reference config.py's defaults
    assert type(opt) is FusedAdamW and opt.max_grad_norm == 5.0
    g = opt.param_groups
    assert (g[0]["lr"], g[0]["betas"], g[0]["eps"], g[0]["weight_decay"], g[1]["weight_decay"]) == (1e-4, (0.9, 0.999), 1e-8, 0.05, 0.0)
    assert build_optimizer(ConfigNode({"TRAIN": {"CLIP_GRAD": 0.0}}), model).max_grad_norm is None
    assert build_optimizer(ConfigNode({}), model, max_grad_norm=None).max_grad_norm is None
    m = build_optimizer(ConfigNode({"OPTIMIZER": {"NAME": "muon", "MUON": {"USE_DISTRIBUTED": True}}}), model, max_grad_norm=1.5)
    assert m.max_grad_norm == 1.5 and type(m.optimizers["MUON"]) is FusedMuon
    mg = m.optimizers["MUON"].param_groups[0]
    assert (mg["momentum"], mg["nesterov"], mg["ns_steps"], mg["lr"], mg["weight_decay"]) == (0.95, True, 5, 1e-4, 0.05)
    # one optimizer is returned bare, with the clip as its own
    lin = torch.nn.Linear(8, 8, bias=False)
    one = build_optimizer(ConfigNode({"OPTIMIZER": {"NAME": "muon"}}), lin)
    assert type(one) is FusedMuon and one.max_grad_norm == 5.0
    emb = torch.nn.Module()
    emb.pos_embed = torch.nn.Parameter(torch.zeros(4, 4))
    one = build_optimizer(ConfigNode({"OPTIMIZER": {"NAME": "muon"}}), emb)
    assert type(one) is FusedAdamW and one.max_grad_norm == 5.0


def test_refusals_name_what_they_refuse(sm):
    model, _ = sm

    def groups(**g):
        return ConfigNode({"OPTIMIZER": {"PARAMETER_GROUPS": dict({"ENABLED": True, "DEFAULT": {"OPTIMIZER": "adamw", "WEIGHT_DECAY": 0.05}}, **g)}})

    with pytest.raises(ValueError, match="overlapping"):
        build_optimizer(groups(A={"FILTER": {"TYPE": "name", "PATTERNS": ["head"]}}, B={"FILTER": {"TYPE": "dimension", "DIMENSIONS": [1]}}), model)
    for kind in ("convolutional", "layer_type", "initialization", "stage_based"):
        with pytest.raises(ValueError, match=kind):
            build_optimizer(groups(A={"FILTER": {"TYPE": "or", "FILTERS": [{"TYPE": kind}]}}), model)
    with pytest.raises(ValueError, match="Unknown optimizer: lion"):
        build_optimizer(ConfigNode({"OPTIMIZER": {"NAME": "lion"}}), model)
    with pytest.raises(ValueError, match="Unknown optimizer: lion"):
        build_optimizer(groups(A={"FILTER": {"TYPE": "name", "PATTERNS": ["head"]}, "OPTIMIZER": "lion"}), model)
    with pytest.raises(ValueError, match="Unknown optimizer: lion"):
        build_optimizer(groups(DEFAULT={"OPTIMIZER": "lion", "WEIGHT_DECAY": 0.0}), model)
    a, b = torch.nn.Parameter(torch.zeros(4, 4)), torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="'X' has its own max_grad_norm"):
        FusedMultiOptimizer({"X": FusedAdamW([a], max_grad_norm=1.0), "Y": FusedSGD([b])})
    with pytest.raises(ValueError, match=r"'Y' \(SGD\) is not a fused optimizer"):
        FusedMultiOptimizer({"X": FusedAdamW([a]), "Y": torch.optim.SGD([b], lr=0.1)}, max_grad_norm=1.0)
    FusedMultiOptimizer({"X": FusedAdamW([a]), "Y": torch.optim.SGD([b], lr=0.1)})  # without a clip any optimizer may take part
    with pytest.raises(ValueError, match="held by both 'X' and 'Y'"):
        FusedMultiOptimizer({"X": FusedAdamW([a, b]), "Y": FusedSGD([b])})
    m = FusedMultiOptimizer({"X": FusedAdamW([a]), "Y": FusedSGD([b])}, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="already held"):
        m.add_param_group({"params": [a], "optimizer_name": "Y"})
    with pytest.raises(ValueError, match="optimizer_name"):
        m.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))]})
    m.add_param_group({"params": [torch.nn.Parameter(torch.zeros(2))], "optimizer_name": "Y", "lr": 0.5})
    assert m.param_groups[-1]["optimizer_name"] == "Y" and m.param_groups[-1]["optimizer_group_idx"] == 1 and m.param_groups[-1]["lr"] == 0.5
    assert repr(m) == "FusedMultiOptimizer (\n  X: FusedAdamW,\n  Y: FusedSGD,\n)"
    # an optimizer clips by its own norm or by a shared one, not both
    with pytest.raises(ValueError, match="max_grad_norm is set"):
        FusedSGD([b], max_grad_norm=1.0).use_shared_clip(torch.zeros(1), 1.0)
    for cls in (FusedAdamW, FusedAdEMAMix, FusedSGD, FusedMuon):
        assert callable(cls.use_shared_clip)


def test_fused_sgd_constructor_follows_torch():
    p = [torch.nn.Parameter(torch.zeros(3))]
    o, t = FusedSGD(p), torch.optim.SGD(p)
    assert set(o.param_groups[0]) == set(t.param_groups[0])
    for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        assert o.param_groups[0][k] == t.param_groups[0][k], k
    assert o.max_grad_norm is None
    o = FusedSGD([{"params": p, "momentum": 0.5}], lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.05, max_grad_norm=2.0)
    assert (o.param_groups[0]["momentum"], o.param_groups[0]["nesterov"], o.param_groups[0]["lr"], o.max_grad_norm) == (0.5, True, 0.1, 2.0)
    for bad in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-0.1), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            FusedSGD(p, **bad)
        with pytest.raises(ValueError):
            torch.optim.SGD(p, **bad)
    with pytest.raises(ValueError, match="maximize"):
        FusedSGD([{"params": p, "maximize": True}])
    with pytest.raises(ValueError, match="Nesterov"):
        FusedSGD([{"params": p, "nesterov": True}], momentum=0.0)
    o = FusedSGD(p, lr=0.1)
    o.step()  # no gradient anywhere: nothing to do, no GPU needed
    p[0].grad = torch.zeros(3)
    with pytest.raises(L.LnxError, match="on the GPU"):
        o.step()


def test_fused_sgd_exchanges_state_dicts_with_torch():
    a, b, c = (torch.nn.Parameter(torch.randn(n)) for n in (5, 7, 3))
    t = torch.optim.SGD([a, b, c], lr=0.1, momentum=0.9, nesterov=True, weight_decay=0.05)
    a.grad, b.grad = torch.randn(5), torch.randn(7)
    t.step()
    sd = t.state_dict()
    sd["state"][1]["momentum_buffer"] = None  # a buffer torch has not created yet
    o = FusedSGD([a, b, c], lr=0.5)
    o.load_state_dict(sd)
    assert o.param_groups[0]["lr"] == 0.1 and o.param_groups[0]["nesterov"] is True
    assert torch.equal(o.state[a]["momentum_buffer"], t.state[a]["momentum_buffer"]) and o.state[b]["momentum_buffer"] is None and c not in o.state
    t2 = torch.optim.SGD([a, b, c], lr=0.3)
    t2.load_state_dict(o.state_dict())
    assert torch.equal(t2.state[a]["momentum_buffer"], t.state[a]["momentum_buffer"]) and t2.param_groups[0]["momentum"] == 0.9


def test_sgd_step_validates_on_the_host():
    """nothing here reaches a launch: every call is refused first, the pointers are never dereferenced"""
    lib = L.lib()
    assert lib.lnx_version() >= 111
    before = lib.lnx_optim_launches()
    fake = 0x10000

    def hyper(**kw):
        h = L.SGDHyper()
        h.ngroups = 2
        for i in range(2):
            h.lr[i], h.momentum[i], h.weight_decay[i] = 0.1, 0.9, 0.05
        h.nesterov[0] = 1
        for k, v in kw.items():
            if k == "ngroups":
                h.ngroups = v
            else:
                getattr(h, k)[1] = v
        return h

    def refused(word, descs=fake, ndesc=2, blocks=2, h=None, no_hyper=False):
        rc = lib.lnx_sgd_step(descs, ndesc, blocks, None if no_hyper else C.byref(h or hyper()), None, 0.0, None)
        err = lib.lnx_last_error()
        assert rc != 0 and b"lnx_sgd_step" in err and word in err, (word, err)

    refused(b"NULL", descs=None)
    refused(b"NULL", no_hyper=True)
    refused(b"ndesc", ndesc=0)
    refused(b"ndesc", ndesc=-3)
    refused(b"total_blocks", blocks=0)
    refused(b"ngroups", h=hyper(ngroups=0))
    refused(b"ngroups", h=hyper(ngroups=L.ADAMW_MAX_GROUPS + 1))
    refused(b"lr", h=hyper(lr=-1e-3))
    refused(b"momentum", h=hyper(momentum=-0.5))
    refused(b"weight_decay", h=hyper(weight_decay=-0.01))
    refused(b"nesterov", h=hyper(nesterov=1, momentum=0.0))
    refused(b"nesterov", h=hyper(nesterov=1, dampening=0.1))
    assert lib.lnx_optim_launches() == before


def test_new_structs_have_the_sizes_the_c_compiler_gives(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"lnx_sgd_hyper": L.SGDHyper, "lnx_muon_step_args": L.MuonStepArgs}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) +
                   '    printf("sumsq %zu\\n", offsetof(lnx_muon_step_args, sumsq));\n    printf("max_norm %zu\\n", offsetof(lnx_muon_step_args, max_norm));\n'
                   '    printf("first %zu\\n", offsetof(lnx_sgd_hyper, first));\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in pairs.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    assert int(got["sumsq"]) == L.MuonStepArgs.sumsq.offset and int(got["max_norm"]) == L.MuonStepArgs.max_norm.offset
    assert int(got["first"]) == L.SGDHyper.first.offset
    assert "lnx_sgd_step" in L.EXPORTS and "lnx_optim_launches" in L.EXPORTS


def filled_multi(order=("B_SGD", "A_ADAMW", "C_MUON")):
    """CPU parameters and hand-filled states: nothing here steps"""
    g = torch.Generator().manual_seed(7)
    ps = {"A_ADAMW": [torch.nn.Parameter(torch.randn(3, 2, generator=g)), torch.nn.Parameter(torch.randn(5, generator=g))],
          "B_SGD": [torch.nn.Parameter(torch.randn(4, generator=g))], "C_MUON": [torch.nn.Parameter(torch.randn(6, 8, generator=g))]}
    made = {"A_ADAMW": FusedAdamW([{"params": ps["A_ADAMW"][:1]}, {"params": ps["A_ADAMW"][1:], "weight_decay": 0.0}], lr=1e-3),
            "B_SGD": FusedSGD(ps["B_SGD"], lr=0.1, momentum=0.9, nesterov=True), "C_MUON": FusedMuon(ps["C_MUON"], lr=0.02)}
    for p in ps["A_ADAMW"]:
        made["A_ADAMW"].state[p] = {"step": 3, "exp_avg": torch.randn(p.shape, generator=g), "exp_avg_sq": torch.rand(p.shape, generator=g)}
    made["B_SGD"].state[ps["B_SGD"][0]] = {"momentum_buffer": torch.randn(4, generator=g)}
    made["C_MUON"].state[ps["C_MUON"][0]] = {"momentum_buffer": torch.randn(6, 8, generator=g)}
    return FusedMultiOptimizer({k: made[k] for k in order}), ps


def test_multi_optimizer_state_dict_round_trip():
    m, ps = filled_multi()
    sd = m.state_dict()
    assert set(sd) == {"_version", "_param_shapes", "optimizers"} and sd["_version"] == 2
    # stable indices: sorted optimizer name, then group, then parameter -- whatever the insertion order
    assert sd["_param_shapes"] == [(3, 2), (5,), (4,), (6, 8)]
    assert list(sd["optimizers"]) == ["B_SGD", "A_ADAMW", "C_MUON"]
    assert sorted(sd["optimizers"]["A_ADAMW"]["state"]) == [0, 1] and list(sd["optimizers"]["B_SGD"]["state"]) == [2] and list(sd["optimizers"]["C_MUON"]["state"]) == [3]
    assert [g["params"] for g in sd["optimizers"]["A_ADAMW"]["param_groups"]] == [[0], [1]]
    assert torch.equal(sd["optimizers"]["A_ADAMW"]["state"][1]["exp_avg"], m.optimizers["A_ADAMW"].state[ps["A_ADAMW"][1]]["exp_avg"])
    assert m.state_dict()["_param_shapes"] == filled_multi(("C_MUON", "B_SGD", "A_ADAMW"))[0].state_dict()["_param_shapes"]

    def fresh():
        f, fp = filled_multi(("C_MUON", "A_ADAMW", "B_SGD"))
        for o in f.optimizers.values():
            o.state.clear()
        f.optimizers["B_SGD"].param_groups[0]["lr"] = 7.0
        return f, fp

    def same_state(f, fp):
        for name, plist in ps.items():
            for p, q in zip(plist, fp[name]):
                a, b = m.optimizers[name].state[p], f.optimizers[name].state[q]
                assert set(a) == set(b)
                for k in a:
                    assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), (name, k)
        assert f.optimizers["B_SGD"].param_groups[0]["lr"] == 0.1

    f, fp = fresh()
    f.load_state_dict(sd)
    same_state(f, fp)
    assert f.param_groups[0]["optimizer_name"] == "C_MUON"  # the tags are the loading optimizer's own
    # string keys (a JSON round trip of the indices)
    f, fp = fresh()
    f.load_state_dict({**sd, "optimizers": {n: {"state": {str(k): v for k, v in o["state"].items()}, "param_groups": o["param_groups"]} for n, o in sd["optimizers"].items()}})
    same_state(f, fp)
    # the legacy form {name: opt.state_dict()}
    f, fp = fresh()
    f.load_state_dict({n: o.state_dict() for n, o in m.optimizers.items()})
    same_state(f, fp)
    # a file as the reference writes it: version 2, every state empty -> fresh state and one warning
    ref_file = {"_version": 2, "_param_shapes": sd["_param_shapes"], "optimizers": {n: {"state": {}, "param_groups": o["param_groups"]} for n, o in sd["optimizers"].items()}}
    f, fp = filled_multi()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        f.load_state_dict(ref_file)
    assert len(w) == 1 and "no optimizer state" in str(w[0].message)
    assert all(len(o.state) == 0 for o in f.optimizers.values())
    # other parameters, or an index of another optimizer, are refused
    with pytest.raises(ValueError, match="_param_shapes"):
        f.load_state_dict({**sd, "_param_shapes": sd["_param_shapes"][:-1]})
    bad = {**sd, "optimizers": {**sd["optimizers"], "B_SGD": {"state": {0: sd["optimizers"]["B_SGD"]["state"][2]}, "param_groups": sd["optimizers"]["B_SGD"]["param_groups"]}}}
    with pytest.raises(ValueError, match="stable index 0"):
        f.load_state_dict(bad)
