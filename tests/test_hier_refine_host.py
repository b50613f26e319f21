"""Hierarchical refinement, the parts that need no GPU: the CPU restatement (tests/hier_refine_ref.py) against what the reference's own
heads computed (tests/golden/hier_refine.npz, written by tests/golden/gen/make_golden_hier_refine.py), the parent / CSR tables derived
from tree matrices, the routing each head type selects, and every host-side refusal of lnx_hier_refine_fwd / lnx_hier_refine_bwd."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import heads as H
from tests import hier_refine_ref as R
from tests.cases import TinyTree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(REPO, "tests", "golden", "hier_refine.npz"), allow_pickle=False)
    keys = [str(k) for k in z["task_keys"]]
    return z, keys


def _t(z, name):
    return torch.from_numpy(z[name])


# ---------------------------------------------------------------------------------------------------- restatement vs the reference
def test_restatement_forward_matches_the_reference_head(fx):
    """fp64 restatement against the reference's fp32 HierarchicalSoftmaxHead outputs.  The values reach |log 1e-10| = 23, fp32 carries
    2^-24 relative per operation over a handful of operations: 1e-5 relative + absolute holds with two orders of margin."""
    z, keys = fx
    bases = [_t(z, f"base_{k}") for k in keys]
    parents = [_t(z, f"parent_{k}") for k in keys[:-1]] + [None]
    outs = R.forward(bases, parents)
    for k, o in zip(keys, outs):
        torch.testing.assert_close(o, _t(z, f"out_{k}").double(), rtol=1e-5, atol=1e-5)
    assert torch.equal(outs[-1], bases[-1].double())
    # the base logits are the recorded classifiers on the recorded input
    for k, b in zip(keys, bases):
        torch.testing.assert_close(_t(z, "x") @ _t(z, f"weight_{k}").t() + _t(z, f"bias_{k}"), b, rtol=1e-5, atol=1e-5)


def test_restatement_backward_matches_the_reference_gradients(fx):
    """The hand-written backward against the gradients autograd gave the reference with respect to each level's base logits (fp32),
    for the probe loss sum_t (out_t * probe_t).sum(): same bound as the forward, the gradients here are O(1..10)."""
    z, keys = fx
    bases = [_t(z, f"base_{k}") for k in keys]
    parents = [_t(z, f"parent_{k}") for k in keys[:-1]] + [None]
    outs = R.forward(bases, parents)
    G = R.backward(outs, [_t(z, f"probe_{k}") for k in keys], parents)
    for k, g in zip(keys, G):
        want = _t(z, f"dbase_{k}").double()
        print(k, "max |restatement - reference| gradient", (g - want).abs().max().item(), "of", want.abs().max().item())
        torch.testing.assert_close(g, want, rtol=1e-5, atol=1e-5)


def test_restatement_routing_modes_match_the_reference(fx):
    z, _ = fx
    x = _t(z, "route_logits")
    soft = R.routing_probs(x, R.SOFT, float(z["soft_temperature"]))
    hard = R.routing_probs(x, R.HARD)
    gumbel = R.routing_probs(x, R.GUMBEL, float(z["gumbel_temperature"]), _t(z, "gumbel_noise"))
    torch.testing.assert_close(soft, _t(z, "route_soft").double(), rtol=1e-5, atol=1e-7)
    assert torch.equal(hard, _t(z, "route_hard").double())
    assert hard[1].argmax().item() == 2 and x[1, 2] == x[1, 4]  # the recorded tie went to the lower index
    torch.testing.assert_close(gumbel, _t(z, "route_gumbel").double(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("storage", [None, torch.bfloat16])
def test_restatement_backward_is_the_derivative_of_its_forward(storage):
    """Hand-written backward against autograd through the same formula in fp64, with every mode, an orphan child, a barren parent and
    a pass-through level; with bf16 storage the rounding is a straight-through step in both."""
    g = torch.Generator().manual_seed(5)
    Cs = [13, 7, 5, 4, 3]
    parents = [R.random_parents(Cs[i], Cs[i + 1], g, orphan_every=5 if i == 0 else 0, barren=(1,) if i == 0 else ()) for i in range(4)] + [None]
    parents[2] = None
    modes, temps = [R.GUMBEL, R.SOFT, R.SOFT, R.HARD, R.SOFT], [0.6, 1.7, 1.0, 1.0, 1.0]
    noises = [torch.randn(4, Cs[1], generator=g)] + [None] * 4
    bases = [torch.randn(4, c, generator=g, dtype=torch.float64, requires_grad=True) for c in Cs]
    douts = [torch.randn(4, c, generator=g, dtype=torch.float64) for c in Cs]
    douts[1] = None
    outs = R.forward([b.detach() for b in bases], parents, modes, temps, noises, storage)
    G = R.backward(outs, douts, parents, modes, temps, noises, storage)
    if storage is not None:
        return  # (values checked on the GPU against this; here: it runs and keeps the shapes)
    live = R.forward(bases, parents, modes, temps, noises)
    sum((o * d).sum() for o, d in zip(live, douts) if d is not None).backward()
    for b, gt in zip(bases, G):
        torch.testing.assert_close(gt, b.grad if b.grad is not None else torch.zeros_like(gt), rtol=1e-10, atol=1e-12)
    assert torch.equal(G[3], douts[3]) and torch.equal(G[4], douts[4])  # nothing crosses the pass-through level or the hard routing


# ---------------------------------------------------------------------------------------------------- tables
def test_parent_and_csr_tables_from_a_tree_matrix():
    m = torch.zeros(5, 9)
    par = [2, 2, 0, -1, 2, 4, 0, 2, -1]  # uneven fan-out (4, 2, 1), parents 1 and 3 without children, two all-zero columns
    for c, p_ in enumerate(par):
        if p_ >= 0:
            m[p_, c] = 1.0
    tab = H.parent_index_from_matrix(m, strict_name="hmatrix_p_c")
    assert tab.dtype == torch.int64 and tab.tolist() == par
    start, idx = H.children_csr(tab, 5)
    assert start.dtype == torch.int32 and idx.dtype == torch.int32
    assert start.tolist() == [0, 2, 2, 6, 6, 7]
    assert idx.tolist() == [2, 6, 0, 1, 4, 7, 5, -1, -1]
    for j in range(5):
        assert idx[start[j]:start[j + 1]].tolist() == [c for c, p_ in enumerate(par) if p_ == j]
    # the same table DevicePredictor derives (one derivation)
    from linnaeus_amd.inference import DevicePredictor

    pred = DevicePredictor(["t_L10", "t_L20"], {"t_L10": 9, "t_L20": 5}, taxonomy_tree={"hmatrix_t_L20_t_L10": m}, consistency=False)
    assert pred.parent_index[0].tolist() == par


def test_bad_matrices_are_refused_by_name():
    two = torch.zeros(3, 4)
    two[0, 1] = two[2, 1] = 1.0
    with pytest.raises(L.LnxError, match="hmatrix_a_b.*more than one 1"):
        H.parent_index_from_matrix(two, strict_name="hmatrix_a_b")
    frac = torch.zeros(3, 4)
    frac[1, 2] = 0.5
    with pytest.raises(L.LnxError, match="hmatrix_a_b.*other than 0 and 1"):
        H.parent_index_from_matrix(frac, strict_name="hmatrix_a_b")
    with pytest.raises(L.LnxError, match=r"\[-1, 3\)"):
        H.children_csr(torch.tensor([0, 3]), 3)


def _heads(head_type, **kw):
    keys, ncls = ["taxa_L10", "taxa_L20", "taxa_L30"], {"taxa_L10": 6, "taxa_L20": 3, "taxa_L30": 2}
    tree = TinyTree({"taxa_L10": {0: 0, 1: 0, 2: 1, 3: 1, 4: 2}, "taxa_L20": {0: 0, 1: 0, 2: 1}}, keys, ncls)
    cfg = {k: dict(TYPE=head_type, **kw) for k in keys}
    return H.configure_classification_heads(cfg, 8, ncls, keys, tree), keys


def test_refinement_object_builds_tables_and_selects_the_routing():
    heads, keys = _heads("ConditionalClassifier", ROUTING_STRATEGY="hard", TEMPERATURE=0.5)
    ref = H.HierarchicalRefinement(heads, keys)
    assert ref.host_tables[0][0].tolist() == [0, 0, 1, 1, 2, -1] and ref.host_tables[1][0].tolist() == [0, 0, 1] and ref.host_tables[2] is None
    assert all(t.dtype == torch.int32 for t in ref.host_tables[0])
    heads.train()
    assert ref.routing(0) == (L.HIER_ROUTE_SOFT, 0.5)  # hard only in eval
    heads.eval()
    assert ref.routing(0) == (L.HIER_ROUTE_HARD, 0.5)
    heads, keys = _heads("ConditionalClassifier", ROUTING_STRATEGY="gumbel", TEMPERATURE=2.0)
    ref = H.HierarchicalRefinement(heads, keys)
    heads.train()
    assert ref.routing(1) == (L.HIER_ROUTE_GUMBEL, 2.0)  # gumbel only in training
    heads.eval()
    assert ref.routing(1) == (L.HIER_ROUTE_SOFT, 2.0)
    heads, keys = _heads("HierarchicalSoftmax")
    ref = H.HierarchicalRefinement(heads, keys)
    assert ref.routing(0) == (L.HIER_ROUTE_SOFT, 1.0)
    with pytest.raises(L.LnxError, match="GPU"):
        ref({k: torch.zeros(2, n) for k, n in zip(keys, (6, 3, 2))})
    with pytest.raises(L.LnxError, match="taxa_L20"):
        ref({"taxa_L10": torch.zeros(2, 6), "taxa_L30": torch.zeros(2, 2)})
    heads["taxa_L10"].hmatrix_taxa_L20_taxa_L10[1, 0] = 1.0  # class 0 under two parents
    with pytest.raises(L.LnxError, match="hmatrix_taxa_L20_taxa_L10"):
        H.HierarchicalRefinement(heads, keys)


# ---------------------------------------------------------------------------------------------------- C ABI
def test_ctypes_mirrors_of_the_refinement_structs_have_the_c_sizes(tmp_path):
    assert L.lib().lnx_version() >= 113
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in L.HIER_REFINE_STRUCTS) +
                   '    printf("modes %d %d %d\\n", LNX_HIER_ROUTE_SOFT, LNX_HIER_ROUTE_HARD, LNX_HIER_ROUTE_GUMBEL);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line, (n, cls) in zip(lines, L.HIER_REFINE_STRUCTS.items()):
        assert line.split() == [n, str(C.sizeof(cls))]
    assert lines[-1].split()[1:] == [str(L.HIER_ROUTE_SOFT), str(L.HIER_ROUTE_HARD), str(L.HIER_ROUTE_GUMBEL)]


def _valid_args():
    """Two levels with every pointer set to a fake address: the checks run on the host and dereference nothing."""
    fake = 0x1000
    a = L.HierRefineArgs()
    a.dtype, a.B, a.n_tasks, a.stats = L.F32, 4, 2, fake
    for t, c in enumerate((6, 3)):
        k = a.level[t]
        k.base = k.out = k.dout = k.dbase = fake
        k.ld = k.ldd = c
        k.C, k.mode, k.temperature = c, L.HIER_ROUTE_SOFT, 1.0
    k = a.level[0]
    k.parent = k.child_start = k.child_idx = fake
    return a


def _refused(fn, a, *words):
    lib = L.lib()
    assert getattr(lib, fn)(C.byref(a), None) == 1, (fn, words)
    msg = lib.lnx_last_error().decode()
    assert msg.startswith(fn + ":") and all(w in msg for w in words), msg


@pytest.mark.parametrize("fn", ["lnx_hier_refine_fwd", "lnx_hier_refine_bwd"])
def test_host_side_refusals(fn):
    lib = L.lib()
    before = lib.lnx_hier_refine_launches()
    assert getattr(lib, fn)(None, None) == 1 and b"NULL arguments" in lib.lnx_last_error()
    for n in (0, -1, L.METRICS_MAX_TASKS + 1):
        a = _valid_args()
        a.n_tasks = n
        _refused(fn, a, f"n_tasks={n}")
    for b in (0, -3):
        a = _valid_args()
        a.B = b
        _refused(fn, a, f"B={b}")
    a = _valid_args()
    a.dtype = 2
    _refused(fn, a, "dtype=2")
    for t in (0, 1):
        a = _valid_args()
        a.level[t].C = 0
        _refused(fn, a, f"level {t}", "C=0")
        a = _valid_args()
        a.level[t].ld = a.level[t].C - 1
        _refused(fn, a, f"level {t}", "ld=")
    for temp in (0.0, -1.0):
        a = _valid_args()
        a.level[0].temperature = temp
        _refused(fn, a, "level 0", "temperature")
    a = _valid_args()
    a.level[0].mode = 3
    _refused(fn, a, "level 0", "unknown routing mode 3")
    a = _valid_args()
    a.level[0].mode = L.HIER_ROUTE_GUMBEL
    _refused(fn, a, "level 0", "gumbel", "noise")
    a = _valid_args()
    a.stats = None
    _refused(fn, a, "stats")
    a = _valid_args()
    a.level[1].out = None
    _refused(fn, a, "level 1", "out")
    # what the coarsest level and a pass-through level do not read is not checked
    a = _valid_args()
    a.level[1].mode, a.level[1].temperature = 9, 0.0
    a.level[0].parent = None
    a.level[0].mode, a.level[0].temperature = 9, -1.0
    a.level[0].ld = a.level[0].C - 1  # (so that the call is still refused, later: nothing may launch in this test)
    _refused(fn, a, "level 0", "ld=")
    assert lib.lnx_hier_refine_launches() == before


def test_host_side_refusals_of_one_direction():
    a = _valid_args()
    a.level[0].base = None
    _refused("lnx_hier_refine_fwd", a, "level 0", "base")
    for name in ("child_start", "child_idx"):
        a = _valid_args()
        setattr(a.level[0], name, None)
        _refused("lnx_hier_refine_bwd", a, "level 0", "CSR")
    a = _valid_args()
    a.level[1].dbase = None
    _refused("lnx_hier_refine_bwd", a, "level 1", "dbase")
    a = _valid_args()
    a.level[0].ldd = 5
    _refused("lnx_hier_refine_bwd", a, "level 0", "ldd=5")
