"""Device metrics without a GPU: the numpy restatement (tests/metrics_ref.py) against the reference's own numbers in
tests/golden/metrics.npz, the two new C-ABI entry points, their argument refusals (checked before any launch) and flush_into."""
import ctypes as C
import os
import shutil
import subprocess
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest

from linnaeus_amd import _lib as L
from tests import metrics_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def load_golden():
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    keys = [str(k) for k in g["task_keys"]]
    batches = []
    for n in range(int(g["n_batches"])):
        batches.append(dict(logits=[g[f"logits_{n}_{t}"] for t in keys], targets=[g[f"target_{n}_{t}"] for t in keys], losses=[g[f"loss_{n}_{t}"] for t in keys]))
    return g, keys, batches


def test_metrics_ref_reproduces_the_reference():
    """Counts equal exactly (the reference's floats hold integers there); ratios equal after the same division; the loss sums the
    reference forms in fp32 (`.sum().item()`, batch mean times B) agree to fp32 rounding of sums of <= 32 terms below 3."""
    g, keys, batches = load_golden()
    T = len(keys)
    counts, sums = R.fresh(T)
    partial_float = 0.0
    for n, b in enumerate(batches):
        c1, s1 = R.fresh(T)
        R.update(c1, s1, b["logits"], b["targets"], losses=b["losses"])
        B = len(b["targets"][0])
        for name in ("chain", "chain_onehot"):
            assert c1[R.CHAIN_N] == B and g[name][n] == c1[R.CHAIN_CORRECT] / c1[R.CHAIN_N]
        for name in ("partial", "partial_onehot"):
            assert g[name][n] == c1[R.PARTIAL_CORRECT] / c1[R.PARTIAL_N]
        partial_float += c1[R.PARTIAL_CORRECT] / c1[R.PARTIAL_N] * B  # what the tracker adds (tracker.py:661)
        counts += c1
        sums += s1
    tr = g["tr_chain"]
    assert tr[0] == counts[R.CHAIN_CORRECT] and tr[1] == counts[R.CHAIN_N] and tr[3] == counts[R.CHAIN_N]
    assert tr[2] == pytest.approx(partial_float, rel=1e-15)
    null_tasks = [str(k) for k in g["null_tasks"]]
    for i, t in enumerate(keys):
        c = counts[R.task_off(i): R.task_off(i) + R.TASK_STRIDE]
        assert g["tr_task_sums_acc1"][i] == c[R.CORRECT1] and g["tr_task_sums_acc3"][i] == c[R.CORRECT3]
        assert g["tr_task_counts_acc1"][i] == c[R.N] and g["tr_task_counts_acc3"][i] == c[R.N] and g["tr_task_counts_loss"][i] == c[R.LOSS_N]
        assert c[R.NULL_N] + c[R.NONNULL_N] == c[R.N] and c[R.CORRECT1] <= c[R.CORRECT3]
        assert g["tr_task_sums_loss"][i] == pytest.approx(sums[R.SUM_STRIDE * i + R.SUM_LOSS], rel=1e-5)
        if t in null_tasks:
            j = null_tasks.index(t)
            assert g["tr_null_sums_acc1"][j] == c[R.NULL_CORRECT1] and g["tr_null_counts_acc1"][j] == c[R.NULL_N] == g["tr_null_counts_loss"][j]
            assert g["tr_non_null_sums_acc1"][j] == c[R.NONNULL_CORRECT1] and g["tr_non_null_counts_acc1"][j] == c[R.NONNULL_N] == g["tr_non_null_counts_loss"][j]
            assert g["tr_null_sums_loss"][j] == pytest.approx(sums[R.SUM_STRIDE * i + R.SUM_NULL_LOSS], rel=1e-5)
            assert g["tr_non_null_sums_loss"][j] == pytest.approx(sums[R.SUM_STRIDE * i + R.SUM_NONNULL_LOSS], rel=1e-5)
    # the fixture exercises what it is for: wrong and right samples, nulls at every rank, samples that are all null
    assert 0 < counts[R.CHAIN_CORRECT] < counts[R.CHAIN_N] and 0 < counts[R.PARTIAL_N] < counts[R.CHAIN_N]
    assert counts[R.PARTIAL_CORRECT] > counts[R.CHAIN_CORRECT] or (g["partial"] != g["chain"]).any()


def test_metrics_ref_ordering_rule():
    nan = float("nan")
    assert list(R.order([1.0, 3.0, 3.0, 2.0])) == [1, 2, 3, 0]
    assert list(R.order([5.0, nan, float("inf"), nan])) == [1, 3, 2, 0]
    c, s = R.fresh(1)
    R.update(c, s, [np.array([[2.0, 2.0, 2.0, 2.0]] * 4)], [np.array([0, 2, 3, 9])])  # all tied: class 0 is top-1, 0..2 the top-3; 9 is outside
    assert c[R.task_off(0) + R.CORRECT1] == 1 and c[R.task_off(0) + R.CORRECT3] == 2
    c, s = R.fresh(2)
    R.update(c, s, [np.array([[0.0, 1.0]]), np.array([[1.0, 0.0]])], [np.array([1]), np.array([1])])  # C = 2: correct3 = correct1
    assert c[R.task_off(0) + R.CORRECT3] == 1 and c[R.task_off(1) + R.CORRECT3] == 0
    assert c[R.CHAIN_CORRECT] == 0 and c[R.PARTIAL_N] == 1 and c[R.PARTIAL_CORRECT] == 0


def test_library_exports_the_metrics_entry_points():
    lib = L.lib()
    assert hasattr(lib, "lnx_metrics_update") and hasattr(lib, "lnx_metrics_table_sizes")
    assert "lnx_metrics_update" in L.EXPORTS and "lnx_metrics_table_sizes" in L.EXPORTS
    nc, ns = C.c_int64(), C.c_int64()
    assert lib.lnx_metrics_table_sizes(4, 5, 7, C.byref(nc), C.byref(ns)) == 0
    assert (nc.value, ns.value) == R.table_sizes(4, 5, 7) == (8 + 32 + 2 * 4 * 12, 16)
    assert lib.lnx_metrics_table_sizes(0, 0, 0, C.byref(nc), C.byref(ns)) != 0 and lib.lnx_metrics_table_sizes(9, 0, 0, C.byref(nc), C.byref(ns)) != 0
    assert lib.lnx_metrics_table_sizes(1, -1, 0, C.byref(nc), C.byref(ns)) != 0
    assert L.metrics_task(3) == R.task_off(3) and L.metrics_subset(4, 5, 1) == R.subset_off(4, 5, 1)


def test_ctypes_mirror_matches_the_header(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "m.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu\\n", sizeof(lnx_metrics_task), sizeof(lnx_metrics_args), offsetof(lnx_metrics_args, task),\n'
                   '           offsetof(lnx_metrics_args, subset_ids), offsetof(lnx_metrics_args, sums));\n'
                   '    printf("%d %d %d %d\\n", (int)LNX_METRICS_TASK(2), (int)LNX_METRICS_SUBSET(4, 5, 1), (int)LNX_METRICS_SUM(3), LNX_METRICS_LOSS_N);\n'
                   "    return 0;\n}\n")
    exe = tmp_path / "m"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(v) for v in out[:5]] == [C.sizeof(L.MetricsTask), C.sizeof(L.MetricsArgs), L.MetricsArgs.task.offset, L.MetricsArgs.subset_ids.offset,
                                         L.MetricsArgs.sums.offset]
    assert [int(v) for v in out[5:]] == [L.metrics_task(2), L.metrics_subset(4, 5, 1), L.METRICS_SUM_STRIDE * 3, L.METRICS_LOSS_N]


def test_update_refuses_bad_arguments_before_any_launch():
    lib = L.lib()
    fake = 4096  # never dereferenced: every call below is refused by the argument checks

    def args(n_tasks=2, C_=10, ld=16):
        a = L.MetricsArgs()
        a.dtype, a.B, a.n_tasks = L.F32, 4, n_tasks
        for t in range(min(max(n_tasks, 0), L.METRICS_MAX_TASKS)):
            a.task[t].logits, a.task[t].ld, a.task[t].C, a.task[t].target = fake, ld, C_, fake
        a.counts, a.sums = fake, fake
        return a

    def refused(a, word):
        assert lib.lnx_metrics_update(C.byref(a), None) != 0
        msg = lib.lnx_last_error()
        assert b"lnx_metrics_update" in msg and word in msg, msg

    refused(args(n_tasks=0), b"n_tasks")
    refused(args(n_tasks=L.METRICS_MAX_TASKS + 1), b"n_tasks")
    refused(args(C_=0), b"C=0")
    refused(args(C_=10, ld=9), b"ld=9")
    a = args()
    a.counts = None
    refused(a, b"NULL")
    a = args()
    a.sums = None
    refused(a, b"NULL")
    a = args()
    a.task[1].target = None
    refused(a, b"task 1")
    a = args()
    a.dtype = 2
    refused(a, b"dtype")
    a = args()
    a.subset_ids[0] = fake  # ids without a bin count
    refused(a, b"n_bins")
    assert lib.lnx_metrics_update(None, None) != 0


class FakeDeviceMetrics:
    """DeviceMetrics with the two tables filled on the host (what compute() / flush_into() read after the one copy)."""

    def __new__(cls, keys, classes, null_tasks, subset_bins, counts, sums):
        import torch

        from linnaeus_amd.metrics import DeviceMetrics

        m = DeviceMetrics(keys, classes, null_tracking_tasks=null_tasks, subset_bins=subset_bins)
        assert (m._n_counts, m._n_sums) == (len(counts), len(sums))
        m.counts, m.sums = torch.from_numpy(counts.copy()), torch.from_numpy(sums.copy())
        return m


def stand_in_tracker(phase):
    tr = SimpleNamespace()
    for name in ("chain_correct", "chain_total", "partial_chain_correct", "partial_chain_total"):
        setattr(tr, name, {phase: 0})
    for name in ("partial_task_sums", "partial_null_sums", "partial_non_null_sums"):
        setattr(tr, name, {phase: defaultdict(lambda: defaultdict(float))})
    for name in ("partial_task_counts", "partial_null_counts", "partial_non_null_counts"):
        setattr(tr, name, {phase: defaultdict(lambda: defaultdict(int))})
    return tr


def test_compute_and_flush_into_on_the_golden_tables():
    """flush_into leaves a stand-in tracker with the reference tracker's accumulators (tests/golden/metrics.npz), except that the
    partial chain pair holds integer counts (the documented difference); compute() names and divides as the tracker does."""
    g, keys, batches = load_golden()
    null_tasks = [str(k) for k in g["null_tasks"]]
    counts, sums = R.fresh(len(keys), 3)
    ids = [np.arange(len(b["targets"][0])) % 4 for b in batches]  # bin 3 does not exist
    for b, i in zip(batches, ids):
        R.update(counts, sums, b["logits"], b["targets"], losses=b["losses"], subset_ids=[i], n_bins=[3])
    # given unsorted: the class sorts by the _L<n> suffix
    m = FakeDeviceMetrics(keys[::-1], {t: int(c) for t, c in zip(keys, g["num_classes"])}, null_tasks, {"rarity": 3}, counts, sums)
    assert m.task_keys == keys
    out = m.compute()
    assert out["chain_accuracy"] == g["tr_chain"][0] / g["tr_chain"][1]
    assert out["partial_chain_accuracy"] == counts[R.PARTIAL_CORRECT] / counts[R.PARTIAL_N]
    for i, t in enumerate(keys):
        assert out[f"acc1_{t}"] == g["tr_task_sums_acc1"][i] / g["tr_task_counts_acc1"][i]
        assert out[f"acc3_{t}"] == g["tr_task_sums_acc3"][i] / g["tr_task_counts_acc3"][i]
        assert out[f"loss_{t}"] == pytest.approx(g["tr_task_sums_loss"][i] / g["tr_task_counts_loss"][i], rel=1e-5)
        assert (f"null_acc1_{t}" in out) == (t in null_tasks) == (f"non_null_loss_{t}" in out)
    for j, t in enumerate(null_tasks):
        assert out[f"null_acc1_{t}"] == g["tr_null_sums_acc1"][j] / g["tr_null_counts_acc1"][j]
        assert out[f"non_null_acc1_{t}"] == g["tr_non_null_sums_acc1"][j] / g["tr_non_null_counts_acc1"][j]
        assert out[f"null_loss_{t}"] == pytest.approx(g["tr_null_sums_loss"][j] / g["tr_null_counts_loss"][j], rel=1e-5)
    sub = out["counts"]["subsets"]["rarity"]
    total = sum(len(i) for i in ids)
    assert sub["out_of_range"] == sum(int((i == 3).sum()) for i in ids) > 0
    assert sum(sub["tasks"][keys[0]]["n"]) == total - sub["out_of_range"]
    assert set(out["subsets"]["rarity"][keys[0]]) == {0, 1, 2}

    tr = stand_in_tracker("val")
    m.flush_into(tr, "val")
    assert (tr.chain_correct["val"], tr.chain_total["val"]) == (g["tr_chain"][0], g["tr_chain"][1])
    assert (tr.partial_chain_correct["val"], tr.partial_chain_total["val"]) == (counts[R.PARTIAL_CORRECT], counts[R.PARTIAL_N])
    for i, t in enumerate(keys):
        for kind in ("acc1", "acc3"):
            assert tr.partial_task_sums["val"][t][kind] == g[f"tr_task_sums_{kind}"][i] and tr.partial_task_counts["val"][t][kind] == g[f"tr_task_counts_{kind}"][i]
        assert tr.partial_task_sums["val"][t]["loss"] == pytest.approx(g["tr_task_sums_loss"][i], rel=1e-5) and tr.partial_task_counts["val"][t]["loss"] == g["tr_task_counts_loss"][i]
    assert sorted(tr.partial_null_sums["val"]) == sorted(null_tasks) == sorted(tr.partial_non_null_counts["val"])
    for j, t in enumerate(null_tasks):
        for name, s_tab, c_tab in (("null", tr.partial_null_sums, tr.partial_null_counts), ("non_null", tr.partial_non_null_sums, tr.partial_non_null_counts)):
            assert s_tab["val"][t]["acc1"] == g[f"tr_{name}_sums_acc1"][j] and c_tab["val"][t]["acc1"] == g[f"tr_{name}_counts_acc1"][j]
            assert s_tab["val"][t]["loss"] == pytest.approx(g[f"tr_{name}_sums_loss"][j], rel=1e-5) and c_tab["val"][t]["loss"] == g[f"tr_{name}_counts_loss"][j]
    # flushed means reset: a second flush adds nothing
    m.flush_into(tr, "val")
    assert tr.chain_total["val"] == g["tr_chain"][1]


def test_compute_with_zero_denominators():
    from linnaeus_amd.metrics import DeviceMetrics

    out = DeviceMetrics(["taxa_L20", "taxa_L10"], {"taxa_L10": 5, "taxa_L20": 9}, null_tracking_tasks=["taxa_L10"]).compute()
    assert out["chain_accuracy"] == 1.0 and out["partial_chain_accuracy"] == 1.0
    assert not any(k.startswith(("acc1_", "acc3_", "loss_", "null_", "non_null_")) for k in out)
