"""lnx_metrics_update / DeviceMetrics on the MI355X against tests/metrics_ref.py (numpy, stable sort).

What is asserted.  Every counter is an integer and must equal the reference's exactly.  The loss sums are double sums of the given
fp32 losses: each addend is exact in double, so the result differs from numpy's float64 sum only by the order of at most B double
additions -- compared at relative 1e-12 (B <= 4099 additions of 2^-53 relative error each stay below 5e-13) -- and must be
bit-identical between two runs.  bf16 logits are compared on the values the kernel is given (the reference sees the same bf16 numbers
converted exactly to float64)."""
import os

import numpy as np
import pytest
import torch

from linnaeus_amd import ops
from linnaeus_amd.metrics import DeviceMetrics
from tests import metrics_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENTINEL = 1.0e30  # in the padding columns: larger than every logit, it would win every argmax if it were read


def padded(x, ld, dtype):
    """x [B, C] on the device as a view of a [B, ld] buffer whose padding holds the sentinel."""
    buf = torch.full((x.shape[0], ld), SENTINEL, dtype=dtype, device="cuda")
    buf[:, : x.shape[1]] = x.to(dtype)
    return buf[:, : x.shape[1]]


def as_f64(t):
    return t.detach().double().cpu().numpy()


def run_kernel(logits, targets, classes, is_null=None, losses=None, subset_ids=(), n_bins=()):
    nb = list(n_bins) + [0, 0]
    nc, ns = ops.metrics_table_sizes(len(logits), nb[0], nb[1])
    counts = torch.zeros(nc, dtype=torch.int64, device="cuda")
    sums = torch.zeros(ns, dtype=torch.float64, device="cuda")
    ops.metrics_update(logits, targets, counts, sums, num_classes=classes, is_null=is_null, losses=losses, subset_ids=subset_ids, n_bins=n_bins)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), sums.cpu().numpy()


def run_ref(logits, targets, classes, is_null=None, losses=None, subset_ids=(), n_bins=()):
    nb = list(n_bins) + [0, 0]
    counts, sums = R.fresh(len(logits), nb[0], nb[1])
    cpu = lambda v: None if v is None else v.cpu().numpy()  # noqa: E731
    R.update(counts, sums, [as_f64(x) for x in logits], [cpu(t) for t in targets], num_classes=classes,
             is_null=None if is_null is None else [cpu(v) for v in is_null], losses=None if losses is None else [cpu(v) for v in losses],
             subset_ids=[cpu(v) for v in subset_ids], n_bins=list(n_bins))
    return counts, sums


def check(got, want, what=""):
    (gc, gs), (wc, ws) = got, want
    assert np.array_equal(gc, wc), (what, np.flatnonzero(gc != wc)[:8], gc[gc != wc][:8], wc[gc != wc][:8])
    np.testing.assert_allclose(gs, ws, rtol=1e-12, atol=0, err_msg=what)


def seeded_case(seed, classes, B, dtype, pad=0, null_frac=0.3, with_loss=True):
    g = torch.Generator().manual_seed(seed)
    logits, targets, losses = [], [], []
    for i, c in enumerate(classes):
        y = torch.randint(0, c, (B,), generator=g)
        y[torch.rand(B, generator=g) < null_frac] = 0
        x = torch.randn(B, c, generator=g)
        x[torch.arange(B), y] += 2.5  # right about half of the time
        ld = c + pad if pad else c
        logits.append(padded(x, ld, dtype) if pad else x.to(dtype).cuda())
        targets.append(y.cuda())
        losses.append((torch.rand(B, generator=g) * 4).cuda() if with_loss else None)
    return logits, targets, losses


def test_kernel_matches_the_reference_on_the_golden_inputs():
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    keys = [str(k) for k in g["task_keys"]]
    classes = [int(c) for c in g["num_classes"]]
    m = DeviceMetrics(keys, classes, null_tracking_tasks=[str(k) for k in g["null_tasks"]])
    counts, sums = R.fresh(len(keys))
    for n in range(int(g["n_batches"])):
        lg = [g[f"logits_{n}_{t}"] for t in keys]
        tg = [g[f"target_{n}_{t}"] for t in keys]
        ls = [g[f"loss_{n}_{t}"] for t in keys]
        R.update(counts, sums, lg, tg, losses=ls)
        m.update({t: torch.from_numpy(v).cuda() for t, v in zip(keys, lg)}, {t: torch.from_numpy(v).cuda() for t, v in zip(keys, tg)},
                 per_sample_losses={t: torch.from_numpy(v).cuda() for t, v in zip(keys, ls)})
    torch.cuda.synchronize()
    check((m.counts.cpu().numpy(), m.sums.cpu().numpy()), (counts, sums), "golden")
    out = m.compute()
    # and with them the reference tracker's own accumulators
    assert out["counts"]["chain_correct"] == g["tr_chain"][0] and out["counts"]["chain_total"] == g["tr_chain"][1]
    for i, t in enumerate(keys):
        assert out[f"acc1_{t}"] == g["tr_task_sums_acc1"][i] / g["tr_task_counts_acc1"][i]
        assert out[f"acc3_{t}"] == g["tr_task_sums_acc3"][i] / g["tr_task_counts_acc3"][i]
        assert out[f"loss_{t}"] == pytest.approx(g["tr_task_sums_loss"][i] / g["tr_task_counts_loss"][i], rel=1e-5)  # the reference sums in fp32


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_sweep_of_task_counts_class_counts_and_batch_sizes(dtype):
    """n_tasks 1..8, C in 1, 2, 3, 20, 1000 and 1500 (above a workgroup's 256 lanes and above 1024), B at the wave / workgroup seams
    and beyond, with and without row padding (ld > C, sentinel in the padding: read once, it would win every argmax)."""
    all_classes = [1, 2, 3, 20, 1000, 1500, 7, 300]
    cases = [(n, all_classes[:n], 65, 0) for n in range(1, 9)]
    cases += [(4, [20, 1000, 3, 1500], B, pad) for B, pad in ((1, 0), (63, 3), (64, 8), (65, 1), (512, 24), (4099, 5))]
    cases += [(2, [1, 2], 512, 1), (1, [1500], 64, 4)]
    for i, (n, classes, B, pad) in enumerate(cases):
        logits, targets, losses = seeded_case(1000 + i, classes, B, dtype, pad=pad)
        check(run_kernel(logits, targets, classes, losses=losses), run_ref(logits, targets, classes, losses=losses), f"case {i}: T={n} C={classes} B={B} pad={pad}")


def test_padding_is_never_read():
    """The same rows contiguous and as views of sentinel-padded buffers (several ld, 16-byte aligned rows and not) give the same table."""
    classes = [20, 1000, 1500]
    for dtype in (torch.float32, torch.bfloat16):
        base, targets, losses = seeded_case(7, classes, 130, dtype)
        want = run_kernel(base, targets, classes, losses=losses)
        for pad in (1, 4, 8, 13):
            views = [padded(x, x.shape[1] + pad, dtype) for x in base]
            assert all(v.stride(0) == c + pad for v, c in zip(views, classes))
            got = run_kernel(views, targets, classes, losses=losses)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (dtype, pad)
        # a logits buffer wider than C with num_classes naming the live columns (the plan's padded logits)
        wide = [padded(x, x.shape[1] + 8, dtype)._base for x in base]
        got = run_kernel(wide, targets, classes, losses=losses)
        assert np.array_equal(got[0], want[0]), dtype


def test_one_hot_targets():
    """[B, C] one-hot / soft rows: class = argmax, null = first column above 0.5 (tracker.py:796-803) -- a soft row whose argmax is
    not 0 but whose first column is 0.6 is null for the split and non-null for the partial chain."""
    keys, classes = ["taxa_L20", "taxa_L10", "taxa_L30"], {"taxa_L10": 20, "taxa_L20": 7, "taxa_L30": 300}
    m = DeviceMetrics(keys, classes, null_tracking_tasks=keys)
    order = m.task_keys
    assert order == ["taxa_L10", "taxa_L20", "taxa_L30"]
    cl = [classes[t] for t in order]
    logits, targets, losses = seeded_case(11, cl, 200, torch.float32)
    onehot = [torch.nn.functional.one_hot(t, c).float() for t, c in zip(targets, cl)]
    onehot[0][:5] = 0.0
    onehot[0][:5, 0] = 0.6
    onehot[0][:5, 3] = 0.7
    idx = [o.argmax(1) for o in onehot]
    nul = [(o[:, 0] > 0.5).to(torch.uint8) for o in onehot]
    m.update(dict(zip(order, logits)), dict(zip(order, onehot)), per_sample_losses=dict(zip(order, losses)))
    torch.cuda.synchronize()
    want = run_ref(logits, idx, cl, is_null=nul, losses=losses)
    check((m.counts.cpu().numpy(), m.sums.cpu().numpy()), want, "one-hot")
    assert want[0][R.task_off(0) + R.NULL_N] >= 5


def test_ties_and_nan_follow_the_stated_order():
    """Integer-valued logits with planted ties (also with the target inside the tie) and one row with NaNs: value descending, index
    ascending, NaN first -- the reference applies the rule with a stable sort."""
    g = torch.Generator().manual_seed(5)
    classes = [3, 20, 300, 1500]
    B = 257
    for dtype in (torch.float32, torch.bfloat16):
        logits, targets = [], []
        for c in classes:
            x = torch.randint(-2, 3, (B, c), generator=g).float()  # five values over up to 1500 columns: ties everywhere
            y = torch.randint(0, c, (B,), generator=g)
            x[torch.arange(0, B, 2), y[0::2]] = 2.0  # every other target shares the maximum
            x[7, :] = 1.0
            x[7, min(5, c - 1)] = float("nan")
            x[7, c - 1] = float("nan")
            y[7] = c - 1  # the second NaN: behind the first, in front of everything else
            x[9, c // 2] = float("nan")
            y[9] = c // 2  # the only NaN: top-1 whatever the numbers are
            x[11, 0] = float("inf")
            x[11, c - 1] = float("nan")
            y[11] = 0  # +inf stays behind the NaN
            logits.append(x.to(dtype).cuda())
            targets.append(y.cuda())
        got, want = run_kernel(logits, targets, classes), run_ref(logits, targets, classes)
        check(got, want, f"ties {dtype}")
        assert 0 < want[0][R.task_off(3) + R.CORRECT1] < want[0][R.task_off(3) + R.CORRECT3] < B


def test_all_null_samples_and_out_of_range_subset_ids():
    classes = [20, 80, 300]
    B = 300
    logits, targets, losses = seeded_case(21, classes, B, torch.float32)
    for t in targets:
        t[:40] = 0  # all-null samples: outside partial_n
    g = torch.Generator().manual_seed(22)
    ids0 = torch.randint(-2, 12, (B,), generator=g).cuda()  # bins 0..9: -2, -1, 10, 11 are out of range
    ids1 = torch.randint(0, 5, (B,), generator=g).cuda()
    ids1[3] = 2 ** 40
    kw = dict(losses=losses, subset_ids=[ids0, ids1], n_bins=[10, 4])
    got, want = run_kernel(logits, targets, classes, **kw), run_ref(logits, targets, classes, **kw)
    check(got, want, "subsets")
    assert want[0][R.PARTIAL_N] <= B - 40 and want[0][R.SUBSET_OOR] > 0 and want[0][R.SUBSET_OOR + 1] > 0
    # every sample all null: the partial pair stays empty, compute() reports 1.0
    m = DeviceMetrics(["a_L1", "a_L2"], [20, 80])
    z = torch.zeros(64, dtype=torch.int64, device="cuda")
    m.update({"a_L1": logits[0][:64], "a_L2": logits[1][:64]}, {"a_L1": z, "a_L2": z})
    out = m.compute()
    assert out["counts"]["partial_chain_total"] == 0 and out["partial_chain_accuracy"] == 1.0 and out["counts"]["chain_total"] == 64
    assert "loss_a_L1" not in out


def test_sums_are_bit_identical_from_run_to_run():
    classes = [20, 1000]
    logits, targets, losses = seeded_case(31, classes, 4099, torch.bfloat16)
    a = run_kernel(logits, targets, classes, losses=losses)
    b = run_kernel(logits, targets, classes, losses=losses)
    assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()
    assert (a[1][[0, 4]] > 0).all()


def test_three_updates_equal_one_on_the_concatenation_and_never_synchronise():
    keys = ["taxa_L10", "taxa_L20", "taxa_L30", "taxa_L40"]
    classes = [20, 80, 300, 1000]
    parts = [seeded_case(40 + i, classes, B, torch.bfloat16, pad=8) for i, B in enumerate((64, 130, 31))]
    ids = [torch.arange(B, device="cuda") % 6 for B in (64, 130, 31)]
    split = DeviceMetrics(keys, classes, null_tracking_tasks=keys[:2], subset_bins={"rarity": 5})
    whole = DeviceMetrics(keys, classes, null_tracking_tasks=keys[:2], subset_bins={"rarity": 5})
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for (lg, tg, ls), i in zip(parts, ids):
            split.update(dict(zip(keys, lg)), dict(zip(keys, tg)), per_sample_losses=dict(zip(keys, ls)), subset_ids={"rarity": i})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    cat = lambda k: {t: torch.cat([p[k][j] for p in parts]) for j, t in enumerate(keys)}  # noqa: E731
    whole.update(cat(0), cat(1), per_sample_losses=cat(2), subset_ids={"rarity": torch.cat(ids)})
    a, b = split.compute(), whole.compute()
    assert np.array_equal(split.counts.cpu().numpy(), whole.counts.cpu().numpy())
    np.testing.assert_allclose(split.sums.cpu().numpy(), whole.sums.cpu().numpy(), rtol=1e-12)
    assert a["chain_accuracy"] == b["chain_accuracy"] and a["subsets"] == b["subsets"] and a["counts"]["subsets"]["rarity"]["out_of_range"] == 36
    want = run_ref([v for v in cat(0).values()], [v for v in cat(1).values()], classes, losses=[v for v in cat(2).values()], subset_ids=[torch.cat(ids)], n_bins=[5])
    check((whole.counts.cpu().numpy(), whole.sums.cpu().numpy()), want, "concatenation")
    split.reset()
    assert int(split.counts.abs().sum()) == 0 and float(split.sums.abs().sum()) == 0.0


def test_end_to_end_on_the_tiny_model():
    """Eval forward of tests/cases.py's tiny model (bf16 and fp32), `outputs` passed straight to DeviceMetrics.update."""
    from linnaeus_amd import build_model
    from oracle import mformer_oracle as O
    from tests.cases import CASES, SEED, make_config, model_state_dict_from_oracle

    spec = CASES["tiny_a"]
    keys = [t for t, _ in spec.heads]
    classes = {t: c for t, c in spec.heads}
    model = build_model(make_config(spec, 64), num_classes=classes)
    model.load_state_dict(model_state_dict_from_oracle(model, O.seeded_state_dict(O.param_shapes(spec), SEED)), strict=True)
    model = model.cuda().eval()
    x, meta = O.seeded_inputs(spec, 16, 64, SEED + 1)
    g = torch.Generator().manual_seed(3)
    targets = {t: torch.randint(0, c, (16,), generator=g).cuda() for t, c in spec.heads}
    for dtype in ("fp32", "bf16"):
        model.set_compute_dtype(dtype)
        with torch.no_grad():
            outputs = model(x.cuda(), meta.cuda())
        m = DeviceMetrics(keys, classes, null_tracking_tasks=keys)
        m.update(outputs, targets)
        out = m.compute()
        lg = [outputs[t] for t in m.task_keys]
        want = run_ref(lg, [targets[t] for t in m.task_keys], [classes[t] for t in m.task_keys])
        check((m.counts.cpu().numpy(), m.sums.cpu().numpy()), want, f"tiny {dtype}")
        if dtype == "fp32":  # (continuous fp32 logits do not tie: torch's own argmax must agree)
            for t in keys:
                assert out[f"acc1_{t}"] == float((outputs[t].argmax(1) == targets[t]).double().mean())
