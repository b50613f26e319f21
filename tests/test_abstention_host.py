"""The abstention phase without a GPU: the fp64 restatement (tests/abstention_ref.py) against the reference's recorded rewards
(tests/golden/abstention.npz, written by tests/golden/gen/make_abstention_golden.py), finding F-a pinned, the torch composition of
linnaeus_amd/rl.py (LNX_ABSTENTION=0) against the restatement on the CPU, and the C ABI: refusals before any launch, struct sizes
against a compiled probe, the exports in both the header and the binding.

The fixture has no GAE arrays: rl_train_abstention.py does not import (its `from linnaeus.config import ... load_config` names a
function linnaeus/config.py does not define, and the module exits), with or without the `gym` stand-in; `gae_from_reference` records
that and the recursion is checked against the restatement only."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import rl
from tests import abstention_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("lnx_abstain_act", "lnx_ppo_advantages", "lnx_ppo_loss_fwd", "lnx_ppo_loss_bwd", "lnx_abstain_launches")
VAL = dict(rtol=2e-5, atol=2e-6)   # tests/test_loss.py: values
GRAD = dict(rtol=2e-4, atol=2e-6)  # tests/test_loss.py: gradients


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "abstention.npz"), allow_pickle=False)


def labels(row):
    return [None if v < 0 else int(v) for v in row]


def test_restatement_reproduces_the_reference_rewards_exactly(golden):
    z = golden
    assert len(z["gt"]) == 216
    seen = set()
    for i in (0, 1):
        table, values = tuple(z[f"table_{i}"]), tuple(z[f"values_{i}"])
        for n, (g, p) in enumerate(zip(z["gt"], z["pred"])):
            preds, gts = labels(p), labels(g)
            seen.update((r, R.outcome_of(a, b)) for r, (a, b) in enumerate(zip(preds, gts)))
            assert R.episode_reward(preds, gts, "simple", "all", table, values) == z[f"simple_list_{i}"][n]
            assert R.episode_reward(preds, gts, "simple", "first", table, values) == z[f"simple_dict_{i}"][n]
            assert R.episode_reward(preds, gts, "outcome", "all", table, values) == z[f"outcome_list_{i}"][n]
            assert R.episode_reward(preds, gts, "outcome", "first", table, values) == z[f"outcome_dict_{i}"][n]
    assert seen == {(r, o) for r in range(3) for o in range(5)}  # every outcome at every rank position


def test_finding_f_a_is_pinned(golden):
    """{"a":[1],"b":[None],"c":[3]} against {"a":[1],"b":[2],"c":[4]} gives 1.0 in the reference (only the first rank is counted);
    the list form {"k":[1,None,3]} / {"k":[1,2,4]} gives -0.5, which is what the docstring intends"""
    preds, gts = [1, None, 3], [1, 2, 4]
    assert R.episode_reward(preds, gts, "simple", "first") == 1.0
    assert R.episode_reward(preds, gts, "simple", "all") == -0.5
    # the same two numbers are in the reference's own record: gt (1, 1, 1), pred (1, None, 2)
    z = golden
    n = [i for i, (g, p) in enumerate(zip(z["gt"], z["pred"])) if tuple(g) == (1, 1, 1) and tuple(p) == (1, -1, 2)]
    assert len(n) == 1 and z["simple_dict_0"][n[0]] == 1.0 and z["simple_list_0"][n[0]] == -0.5


def forcing_logits(pred, C_=4):
    """rows whose arg-max is the wanted action (None -> class 0, the abstain index)"""
    x = torch.zeros(len(pred), C_)
    x[torch.arange(len(pred)), torch.tensor([0 if v < 0 else int(v) for v in pred])] = 5.0
    return x


@pytest.mark.parametrize("kind", ["simple", "outcome"])
@pytest.mark.parametrize("ranks", ["all", "first"])
def test_composition_rewards_equal_the_reference_record(golden, monkeypatch, kind, ranks):
    """multitask mode, greedy, logits that force the recorded predictions: the composition's rewards are the reference's numbers"""
    monkeypatch.setenv("LNX_ABSTENTION", "0")
    z = golden
    logits = [forcing_logits(z["pred"][:, r]) for r in range(3)]
    targets = [torch.from_numpy(np.where(z["gt"][:, r] < 0, 0, z["gt"][:, r])) for r in range(3)]
    got = rl.act(logits, targets, None, "multitask", True, rl.AbstentionReward(kind, ranks))
    want = z[f"{kind}_{'list' if ranks == 'all' else 'dict'}_0"]
    assert torch.equal(got.reward.double(), torch.from_numpy(want))


def random_problem(seed, B=37, Cs=(9, 5, 7, 3), scale=2.0):
    g = torch.Generator().manual_seed(seed)
    logits = [torch.randn(B, c, generator=g) * scale for c in Cs]
    targets = [torch.randint(0, c, (B,), generator=g) for c in Cs]
    for r, t in enumerate(targets):
        t[torch.rand(B, generator=g) < 0.3] = 0
        t[r::len(Cs)][:1] = 0  # a null at every rank position
    u = torch.rand(B, len(Cs), generator=g)
    return logits, targets, u


@pytest.mark.parametrize("mode", ["multitask", "sequential"])
@pytest.mark.parametrize("kind,ranks", [("simple", "all"), ("simple", "first"), ("outcome", "all"), ("outcome", "first")])
def test_composition_equals_the_restatement_on_the_cpu(monkeypatch, mode, kind, ranks):
    monkeypatch.setenv("LNX_ABSTENTION", "0")
    logits, targets, u = random_problem(11)
    counts = torch.zeros(L.ABSTAIN_COUNTS, dtype=torch.int64)
    got = rl.act(logits, targets, u, mode, False, rl.AbstentionReward(kind, ranks), counts=counts)
    ref = R.rollout_ref(logits, targets, u, mode, kind=kind, ranks=ranks, forced_actions=got.actions)
    far = (ref["margin"] > 1e-5) & got.taken.bool()
    assert torch.equal(got.actions.long()[far], ref["own_actions"][far]) and far.float().mean() > 0.5
    assert torch.equal(got.taken, ref["taken"]) and torch.equal(got.length, ref["length"])
    assert torch.equal(got.actions.long(), ref["actions"])
    torch.testing.assert_close(got.logp.double(), ref["logp"], **VAL)
    torch.testing.assert_close(got.entropy.double(), ref["entropy"], **VAL)
    assert torch.equal(got.reward.double(), ref["reward"])
    assert counts.tolist() == ref["counts"]
    if mode == "sequential":
        assert set(got.length.tolist()) == {1, 2, 3, 4}  # episodes of every length

    value = torch.randn(len(got.reward), generator=torch.Generator().manual_seed(5))
    adv, ret, n = rl.advantages(got.reward, value, got.length, mode, 4, 0.99, 0.95)
    adv_ref, ret_ref, n_ref = R.advantages_ref(got.reward.numpy(), value.numpy(), got.length.numpy(), mode, 4, 0.99, 0.95)
    assert int(n) == n_ref
    torch.testing.assert_close(adv.double(), adv_ref, **VAL)
    torch.testing.assert_close(ret.double(), ret_ref, **VAL)

    lg = [x.clone().requires_grad_(True) for x in logits]
    v = value.clone().requires_grad_(True)
    logp_old = got.logp + 0.3 * torch.randn(got.logp.shape, generator=torch.Generator().manual_seed(6)) * got.taken
    total, stats = rl.ppo_loss(lg, v, got.actions, got.taken, logp_old, adv, ret, mode, 0.2, 0.5, 0.01)
    total.backward()
    want, dl, dv = R.ppo_loss_ref(logits, value, got.actions, got.taken, logp_old, adv, ret, mode, 0.2, 0.5, 0.01)
    for k, w in want.items():
        torch.testing.assert_close(float(stats[k]), w, **VAL)
    assert 0.0 < want["clip_frac"] < 1.0
    for x, d in zip(lg, dl):
        torch.testing.assert_close(x.grad.double(), d, **GRAD)
    torch.testing.assert_close(v.grad.double(), dv, **GRAD)


def test_gae_restatement_on_whole_episodes(golden):
    """a complete episode: the value after its last step is multiplied by 1 - done = 0, so last_value never enters"""
    rewards, values, dones = np.array([0.0, 0.0, 1.5]), np.full(3, 0.25), np.array([0.0, 0.0, 1.0])
    a0, r0 = R.gae_and_returns(rewards, values, dones, 0.0, 0.99, 0.95)
    a1, r1 = R.gae_and_returns(rewards, values, dones, 1e6, 0.99, 0.95)
    assert np.array_equal(a0, a1) and np.array_equal(r0, r1)
    d2 = 1.5 - 0.25
    d1 = 0.99 * 0.25 - 0.25
    want = [d1 + 0.99 * 0.95 * (d1 + 0.99 * 0.95 * d2), d1 + 0.99 * 0.95 * d2, d2]
    np.testing.assert_allclose(a0, want, rtol=1e-14)
    np.testing.assert_allclose(r0, np.array(want) + 0.25, rtol=1e-14)
    if int(golden["gae_from_reference"]):  # (absent here: see the module docstring)
        z = golden
        a, r = R.gae_and_returns(z["gae_rewards"], z["gae_values"], z["gae_dones"], 0.0, float(z["gae_gamma"]), float(z["gae_lambda"]))
        np.testing.assert_allclose(a, z["gae_adv"], rtol=1e-12)
        np.testing.assert_allclose(r, z["gae_ret"], rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def declared_symbols():
    src = open(os.path.join(REPO, "include", "lnx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return set(re.findall(r"\b(lnx_[a-z0-9_]+)\s*\(", src))


def test_new_exports_are_in_the_header_the_binding_and_the_library():
    lib = L.lib()
    for name in NEW_EXPORTS:
        assert name in declared_symbols(), name
        assert name in L.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.lnx_version() >= 116
    assert lib.lnx_abstain_launches() >= 0


def test_struct_sizes_against_the_c_compiler(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = L.ABSTENTION_STRUCTS
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in pairs.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
        assert C.sizeof(cls) < 4096, n  # passed by value to the kernels


FAKE = 0x1000  # never dereferenced: every call below is refused on the host, before any launch


def act_args():
    a = L.AbstainActArgs()
    a.dtype, a.B, a.R, a.mode = L.F32, 4, 2, L.ABSTAIN_SEQUENTIAL
    a.u = a.actions = a.logp = a.entropy = a.taken = a.length = a.reward = FAKE
    for r in range(2):
        k = a.rank[r]
        k.logits, k.ld, k.C, k.target = FAKE, 8, 8, FAKE
    return a


def loss_args():
    a = L.PpoLossArgs()
    a.dtype, a.B, a.R, a.mode, a.clip_eps = L.F32, 4, 2, L.ABSTAIN_MULTITASK, 0.2
    a.actions = a.taken = a.logp_old = a.adv = a.ret = a.value = a.ws = a.out = a.dvalue = FAKE
    for r in range(2):
        k = a.rank[r]
        k.logits, k.ld, k.C, k.dlogits, k.ldd = FAKE, 8, 8, FAKE, 8
    return a


def adv_args():
    a = L.PpoAdvArgs()
    a.B, a.R, a.mode = 4, 2, L.ABSTAIN_SEQUENTIAL
    a.reward = a.value = a.length = a.adv = a.ret = a.n_trans = FAKE
    return a


def refused(fn, args, *more):
    lib = L.lib()
    before = lib.lnx_abstain_launches()
    rc = getattr(lib, fn)(C.byref(args), *more, None)
    assert lib.lnx_abstain_launches() == before, fn  # nothing was launched
    return rc != 0 and fn.encode() in lib.lnx_last_error()


def set_field(obj, path, value):
    *head, last = path
    for p in head:
        obj = obj[p] if isinstance(p, int) else getattr(obj, p)
    setattr(obj, last, value)


@pytest.mark.parametrize("path,value", [
    (("R",), 0), (("R",), 9), (("B",), 0), (("B",), -3), (("dtype",), 2), (("mode",), 2), (("reward_kind",), 2), (("reward_ranks",), -1),
    (("u",), None), (("actions",), None), (("logp",), None), (("entropy",), None), (("taken",), None), (("length",), None), (("reward",), None),
    (("rank", 1, "C"), 0), (("rank", 1, "ld"), 7), (("rank", 0, "logits"), None), (("rank", 1, "target"), None),
    (("rank", 0, "abstain_index"), 8), (("rank", 0, "abstain_index"), -1), (("rank", 1, "null_index"), 8), (("rank", 1, "null_index"), -1),
])
def test_act_refuses_on_the_host(path, value):
    a = act_args()
    set_field(a, path, value)
    assert refused("lnx_abstain_act", a), path
    assert refused("lnx_abstain_act", L.AbstainActArgs())


def test_act_takes_a_null_u_with_greedy_only():
    lib = L.lib()
    assert lib.lnx_abstain_act(None, None) != 0 and b"NULL arguments" in lib.lnx_last_error()
    a = act_args()
    a.u, a.greedy, a.B = None, 1, 0  # greedy lifts the need for u: the refusal that remains is B = 0
    assert refused("lnx_abstain_act", a) and b"B=0" in lib.lnx_last_error()


@pytest.mark.parametrize("path,value", [
    (("R",), 0), (("R",), 9), (("B",), 0), (("mode",), 5), (("reward",), None), (("value",), None), (("length",), None), (("adv",), None),
    (("ret",), None), (("n_trans",), None),
])
def test_advantages_refuse_on_the_host(path, value):
    a = adv_args()
    set_field(a, path, value)
    assert refused("lnx_ppo_advantages", a), path


@pytest.mark.parametrize("fn", ["lnx_ppo_loss_fwd", "lnx_ppo_loss_bwd"])
@pytest.mark.parametrize("path,value", [
    (("R",), 0), (("R",), 9), (("B",), 0), (("dtype",), 3), (("mode",), -1), (("clip_eps",), -0.1), (("actions",), None), (("taken",), None),
    (("logp_old",), None), (("adv",), None), (("ret",), None), (("value",), None), (("ws",), None), (("out",), None),
    (("rank", 1, "C"), 0), (("rank", 0, "ld"), 7), (("rank", 1, "logits"), None), (("rank", 0, "ldd"), 7),
])
def test_loss_refuses_on_the_host(fn, path, value):
    a = loss_args()
    set_field(a, path, value)
    more = (C.c_void_p(FAKE),) if fn.endswith("bwd") else ()
    assert refused(fn, a, *more), path


def test_loss_backward_needs_go_and_an_output():
    a = loss_args()
    assert refused("lnx_ppo_loss_bwd", a, None) and b"go_dev" in L.lib().lnx_last_error()
    a.dvalue = None
    for r in range(2):
        a.rank[r].dlogits = None
    assert refused("lnx_ppo_loss_bwd", a, C.c_void_p(FAKE))


def test_python_layer_validates():
    with pytest.raises(ValueError):
        rl.AbstentionReward("dense")
    with pytest.raises(ValueError):
        rl.AbstentionReward("simple", "last")
    r = rl.AbstentionReward()
    assert r.table == list(R.SIMPLE_DEFAULT) and r.outcome == list(R.OUTCOME_DEFAULT)
    res = rl.results_from_counts([0] * L.ABSTAIN_COUNTS, ["taxa_L20", "taxa_L10"])
    assert res["mean_reward"] == 0 and res["abst_rate/taxa_L20"] == 0 and "missed_abst_count/taxa_L10" in res
