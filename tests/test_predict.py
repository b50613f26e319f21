"""lnx_predict / DevicePredictor without a GPU: the numpy restatement against the reference's recorded results, the parent tables from
their three sources, argument handling, the ctypes mirrors against the C compiler, and every refusal the launcher makes on the host."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from linnaeus_amd import DevicePredictor
from linnaeus_amd import _lib as L
from tests import predict_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "predict.npz")


def fixture():
    g = np.load(GOLDEN)
    keys = [str(k) for k in g["task_keys"]]
    return g, keys, [int(c) for c in g["num_classes"]]


class DuckTree:
    """get_parent alone, as DevicePredictor needs it."""

    def __init__(self, keys, tables):
        self.keys, self.tables = keys, tables

    def get_parent(self, node):
        key, c = node
        i = self.keys.index(key)
        if i + 1 >= len(self.keys) or self.tables[i][c] < 0:
            return None
        return (self.keys[i + 1], int(self.tables[i][c]))


def test_restatement_reproduces_the_reference_results():
    """predict_ref on the fixture's logits against what the reference's enforce_hierarchical_consistency returned for them: ids and
    counts equal, probabilities to 1e-6 (the reference's come from an fp32 softmax), with and without the consistency pass."""
    g, keys, classes = fixture()
    logits = [g[f"logits_{k}"] for k in keys]
    parents = [g[f"parent_{k}"] for k in keys[:-1]] + [None]
    id_maps = [g[f"taxon_id_{k}"] for k in keys]
    ids, probs, count, flags = R.predict(logits, parents, 5, null_index=0, id_maps=id_maps, k_per_sample=g["k"])
    assert np.array_equal(ids, g["ids"]) and np.array_equal(count, g["count"])
    np.testing.assert_allclose(probs, g["probs"], rtol=0, atol=1e-6)
    assert (probs[flags != 0][:, 0] == 1.0).all() and (count[flags != 0] == 1).all()
    # what each scenario of the generator must come out as: consistent samples carry no flag; a break at a rank flags 2 there and 1 below
    sc = g["scenario"]
    assert (flags[sc == 0] == 0).all() and set(np.unique(flags)) == {0, 1, 2}
    for s, t_break in ((1, 2), (2, 1), (3, 0), (5, 2), (6, 1), (7, 0)):
        f = flags[sc == s]
        assert (f[:, t_break] == 2).all() and (f[:, :t_break] == 1).all() and (f[:, t_break + 1:] == 0).all(), s
    assert (flags[sc == 4][:, :3] == 1).all() and (flags[sc == 4][:, 3] == 0).all()  # a null coarsest keeps its list, all below go
    assert (count[sc == 4][:, 3] == np.minimum(g["k"][sc == 4], 3)).all()
    ids, probs, count, flags = R.predict(logits, parents, 5, null_index=0, id_maps=id_maps, k_per_sample=g["k"], consistency=False)
    assert np.array_equal(ids, g["raw_ids"]) and np.array_equal(count, g["raw_count"]) and not flags.any()
    np.testing.assert_allclose(probs, g["raw_probs"], rtol=0, atol=1e-6)


def test_restatement_order_and_softmax_on_special_values():
    assert R.order([1.0, 3.0, 3.0, float("nan"), -0.0, 0.0, float("inf")]).tolist() == [3, 6, 1, 2, 0, 4, 5]
    p = R.softmax([0.0, float("-inf"), 0.0])
    assert p.tolist() == [0.5, 0.0, 0.5]
    assert np.isnan(R.softmax([0.0, float("nan")])).all()
    # a task without a null index is flagged but kept, and its own top-1 stays the node its children are held against
    ids, probs, count, flags = R.predict([np.array([[0.0, 5.0, 1.0]]), np.array([[0.0, 1.0, 5.0]]), np.array([[5.0, 0.0]])],
                                         [np.array([-1, 2, 1]), np.array([-1, 1, 1]), None], 2, null_index=[0, None, 0])
    assert flags.tolist() == [[0, 1, 0]] and count.tolist() == [[2, 2, 2]] and ids[0, :, 0].tolist() == [1, 2, 0]


def test_parent_tables_from_the_three_sources_agree():
    g, keys, classes = fixture()
    want = [g[f"parent_{k}"] for k in keys[:-1]]
    from_tree = DevicePredictor(keys, classes, taxonomy_tree=DuckTree(keys, want))
    from_explicit = DevicePredictor(list(reversed(keys)), dict(zip(keys, classes)), parent_index={k: torch.from_numpy(w).long() for k, w in zip(keys, want)})
    hm = {}
    for i, w in enumerate(want):  # [n_parent, n_child] 0/1 membership, as TaxonomyTree.build_hierarchy_matrices makes it
        m = torch.zeros(classes[i + 1], classes[i])
        for c, p in enumerate(w):
            if p >= 0:
                m[p, c] = 1.0
        hm[f"hmatrix_{keys[i + 1]}_{keys[i]}"] = m
    from_dict = DevicePredictor(keys, classes, taxonomy_tree=hm)
    head = torch.nn.Module()
    for name, m in hm.items():
        head.register_buffer(name, m)
    from_buffers = DevicePredictor(keys, classes, taxonomy_tree=head)
    for p in (from_tree, from_explicit, from_dict, from_buffers):
        assert p.task_keys == keys and p.num_classes == classes  # sorted finest first whatever order they came in
        assert p.parent_index[-1] is None
        for got, w in zip(p.parent_index[:-1], want):
            assert got.dtype == torch.int32 and got.tolist() == w.tolist()
    with pytest.raises(L.LnxError, match="parent table"):
        DevicePredictor(keys, classes, parent_index={keys[0]: torch.zeros(classes[0], dtype=torch.long)})  # the other ranks are missing
    DevicePredictor(keys, classes, consistency=False)  # no tables needed
    with pytest.raises(L.LnxError, match="parent table"):
        DevicePredictor(keys, classes, parent_index={k: torch.full((c,), 99) for k, c in zip(keys, classes)})
    with pytest.raises(L.LnxError, match="not both"):
        DevicePredictor(keys, classes, taxonomy_tree=hm, parent_index={})


def test_null_index_top_k_and_id_map_arguments():
    g, keys, classes = fixture()
    kw = dict(parent_index={k: g[f"parent_{k}"] for k in keys[:-1]})
    assert DevicePredictor(keys, classes, **kw).null_index == [0, 0, 0, 0]
    assert DevicePredictor(keys, classes, null_index=2, **kw).null_index == [2, 2, 2, 2]
    assert DevicePredictor(keys, classes, null_index={keys[1]: None, keys[2]: 1}, **kw).null_index == [0, None, 1, 0]
    with pytest.raises(L.LnxError, match="null index"):
        DevicePredictor(keys, classes, null_index=3, **kw)  # the coarsest rank has 3 classes
    with pytest.raises(L.LnxError, match="unknown"):
        DevicePredictor(keys, classes, null_index={"taxa_L99": 0}, **kw)
    for bad in (0, 17):
        with pytest.raises(L.LnxError, match="top_k"):
            DevicePredictor(keys, classes, top_k=bad, **kw)
    p = DevicePredictor(keys, classes, top_k=5, idx_to_taxon_id={keys[0]: {i: 2 ** 40 + i for i in range(classes[0])}, keys[3]: g[f"taxon_id_{keys[3]}"]}, **kw)
    assert p.id_maps[0].tolist()[-1] == 2 ** 40 + classes[0] - 1 and p.id_maps[1] is None and p.id_maps[3].dtype == torch.int64
    with pytest.raises(L.LnxError, match="id map"):
        DevicePredictor(keys, classes, idx_to_taxon_id={keys[0]: [1, 2]}, **kw)
    cpu = torch.device("cpu")
    assert p._k_args(None, 4, cpu) == (5, None) and p._k_args(3, 4, cpu) == (3, None)
    K, kps = p._k_args([1, None, 7, 3], 4, cpu)
    assert K == 7 and kps.dtype == torch.int32 and kps.tolist() == [1, 5, 7, 3]
    K, kps = p._k_args(torch.tensor([2, 4]), 2, cpu)
    assert K == 4 and kps.tolist() == [2, 4]
    for bad in (0, 17, [1, 99], torch.tensor([0, 1])):
        with pytest.raises(L.LnxError, match="top_k"):
            p._k_args(bad, 2, cpu)
    with pytest.raises(L.LnxError, match="top_k"):
        p._k_args([1, 2, 3], 2, cpu)
    with pytest.raises(L.LnxError, match="dict-valued"):
        p.predict_logits({k: {"x": torch.zeros(2, c)} for k, c in zip(keys, classes)})
    with pytest.raises(L.LnxError, match="no CPU fallback"):
        p.predict_logits({k: torch.zeros(2, c) for k, c in zip(keys, classes)})


def test_to_results_orders_coarsest_first_and_cuts_at_count():
    p = DevicePredictor(["a_L10", "a_L20"], [3, 2], consistency=False)
    pred = {"ids": torch.tensor([[[7, 8, -1], [5, -1, -1]]]), "probs": torch.tensor([[[0.75, 0.25, 0.0], [1.0, 0.0, 0.0]]]),
            "count": torch.tensor([[2, 1]], dtype=torch.int32), "flags": torch.zeros(1, 2, dtype=torch.int32)}
    assert p.to_results(pred) == [[("a_L20", [(5, 1.0)]), ("a_L10", [(7, 0.75), (8, 0.25)])]]


def test_ctypes_mirrors_have_the_sizes_the_c_compiler_gives(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    pairs = {"lnx_predict_task": L.PredictTask, "lnx_predict_args": L.PredictArgs}
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in pairs) +
                   '    printf("off_task %zu\\n", offsetof(lnx_predict_args, task));\n    printf("off_ids %zu\\n", offsetof(lnx_predict_args, ids));\n'
                   '    printf("max_k %d\\n", LNX_PREDICT_MAX_K);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in pairs.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    assert int(got["off_task"]) == L.PredictArgs.task.offset and int(got["off_ids"]) == L.PredictArgs.ids.offset
    assert int(got["max_k"]) == L.PREDICT_MAX_K


def valid_args():
    """Arguments that pass every host check (the pointers are never dereferenced: each test below breaks one field, and B = 0 returns
    before a launch)."""
    fake = C.c_void_p(0x1000)
    a = L.PredictArgs()
    a.dtype, a.B, a.n_tasks, a.K, a.consistency = L.BF16, 0, 2, 5, 1
    for t in range(2):
        a.task[t].logits, a.task[t].ld, a.task[t].C, a.task[t].null_index = fake, 8, 7, 0
    a.task[0].parent = fake
    a.ids = a.probs = a.count = a.flags = fake
    return a


def test_lnx_predict_refuses_bad_arguments_without_a_gpu():
    lib = L.lib()
    assert lib.lnx_version() >= 104
    assert lib.lnx_predict(C.byref(valid_args()), None) == 0, lib.lnx_last_error()  # B = 0: accepted, nothing launched

    def refused(word, **fields):
        a = valid_args()
        for name, v in fields.items():
            if name.startswith("task0_"):
                setattr(a.task[0], name[6:], v)
            elif name.startswith("task1_"):
                setattr(a.task[1], name[6:], v)
            else:
                setattr(a, name, v)
        assert lib.lnx_predict(C.byref(a), None) != 0, fields
        assert word.encode() in lib.lnx_last_error(), (fields, lib.lnx_last_error())

    refused("dtype", dtype=2)
    refused("K=", K=0)
    refused("K=", K=L.PREDICT_MAX_K + 1)
    refused("n_tasks", n_tasks=0)
    refused("n_tasks", n_tasks=L.METRICS_MAX_TASKS + 1)
    refused("C=", task1_C=0)
    refused("ld=", task0_ld=6)
    for out in ("ids", "probs", "count", "flags"):
        refused("NULL output", **{out: None})
    refused("parent", task0_parent=None)
    a = valid_args()  # without the consistency pass no parent table is needed, and the coarsest task never needs one
    a.consistency, a.task[0].parent = 0, None
    assert lib.lnx_predict(C.byref(a), None) == 0, lib.lnx_last_error()
    assert lib.lnx_predict(None, None) != 0
