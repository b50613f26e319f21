"""lnx_predict / DevicePredictor on the MI355X against tests/predict_ref.py (numpy float64, stable sort) run on the same stored values.

What is asserted.  ids, count and flags are integers and must equal the reference's; entries at or beyond count are exactly (-1, 0);
a nullified probability is exactly 1.0.  Every other probability is within rtol 2e-5 of the float64 softmax: a lane sums at most
ceil(4099 / 64) = 65 terms, six merge steps follow, each operation within 2^-24 relative, plus a few ulp of expf -- about 5e-6 at
worst, with a factor 4 of room.  bf16 logits are compared on the values the kernel is given (bf16 -> float64 is exact).  Every output
tensor sits between guard rows that must come back untouched.  The largest error seen is printed (run with -s)."""
import os

import numpy as np
import pytest
import torch

from linnaeus_amd import DevicePredictor, ops
from tests import predict_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 2e-5
GUARD = 64
SEEN = {"max_rel": 0.0}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def place(x, dtype, layout):
    """x [B, C] (CPU fp32) on the device as `dtype`: "contig"; "padded": a view of a [B, C + 3] buffer; "offset": the same, starting one
    element into the allocation, so that the first row is not 16-byte aligned.  The padding holds +inf: read once, it would win every
    arg-best and turn every sum into inf."""
    B, C = x.shape
    if layout == "contig":
        return x.to(dtype).cuda()
    ld, off = C + 3, int(layout == "offset")
    buf = torch.full((off + B * ld,), float("inf"), dtype=dtype, device="cuda")
    view = buf[off:].view(B, ld)[:, :C]
    view.copy_(x.to(dtype))
    assert view.stride(0) == ld and (off == 0 or view.data_ptr() % 16 != 0)
    return view


def guarded(shape, dtype, fill):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD: GUARD + n].view(*shape)


def run_kernel(logits, parents, K, **kw):
    """One launch into guarded outputs -> numpy (ids, probs, count, flags)."""
    B, T = logits[0].shape[0], len(logits)
    fills = ((torch.int64, -77), (torch.float32, -77.0), (torch.int32, -77), (torch.int32, -77))
    bufs = [guarded(s, dt, f) for s, (dt, f) in zip(((B, T, K), (B, T, K), (B, T), (B, T)), fills)]
    out = ops.predict_topk(logits, parents, K=K, out=tuple(v for _, v in bufs), **kw)
    torch.cuda.synchronize()
    for (buf, _), (_, f) in zip(bufs, fills):
        assert bool((buf[:GUARD] == f).all()) and bool((buf[-GUARD:] == f).all()), "guard rows were written"
    return tuple(o.cpu().numpy() for o in out)


def run_ref(logits, parents, K, null_index=0, id_maps=None, k_per_sample=None, consistency=True, num_classes=None):
    cpu = lambda v: v if v is None or isinstance(v, np.ndarray) else v.cpu().numpy()  # noqa: E731
    lg = [x.detach().double().cpu().numpy()[:, : (num_classes[t] if num_classes else x.shape[1])] for t, x in enumerate(logits)]
    return R.predict(lg, [cpu(p) for p in parents], K, null_index=null_index, id_maps=None if id_maps is None else [cpu(m) for m in id_maps],
                     k_per_sample=cpu(k_per_sample), consistency=consistency)


def check(got, want, what=""):
    (gi, gp, gc, gf), (wi, wp, wc, wf) = got, want
    assert np.array_equal(gi, wi), (what, "ids", np.argwhere(gi != wi)[:6].tolist(), gi[gi != wi][:6], wi[gi != wi][:6])
    assert np.array_equal(gc, wc) and np.array_equal(gf, wf), (what, "count / flags")
    K = gi.shape[2]
    beyond = np.arange(K)[None, None, :] >= gc[:, :, None]
    assert (gp[beyond] == 0.0).all() and (gi[beyond] == -1).all(), (what, "entries beyond count")
    nullified = (gf != 0) & (gc == 1) & (wp[:, :, 0] == 1.0)
    assert (gp[:, :, 0][nullified] == 1.0).all(), (what, "nullified probability")
    assert np.array_equal(np.isnan(gp), np.isnan(wp)), (what, "NaN probabilities")
    live = ~beyond & ~np.isnan(wp)
    rel = np.abs(gp[live].astype(np.float64) - wp[live]) / np.maximum(wp[live], 1e-300)
    rel = np.where(wp[live] == 0.0, np.where(gp[live] == 0.0, 0.0, np.inf), rel)
    if rel.size:
        SEEN["max_rel"] = max(SEEN["max_rel"], float(rel.max()))
        print(f"[predict] {what}: largest relative probability error {rel.max():.3e} (run so far {SEEN['max_rel']:.3e})")
        assert rel.max() <= RTOL, (what, float(rel.max()))


# ---------------------------------------------------------------------------------------------------------------------
SEAM_C = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4099]
_seam_cache = {}


def seam_rows(dtype):
    """One set of stored values per dtype, B = 5 rows per class count, and its reference per K -- computed once, shared by the layouts."""
    if dtype not in _seam_cache:
        g = torch.Generator().manual_seed(101)
        rows = [(torch.randn(5, c, generator=g) * 3.0).to(dtype).float() for c in SEAM_C]
        _seam_cache[dtype] = (rows, {})
    return _seam_cache[dtype]


@DTYPES
@pytest.mark.parametrize("layout", ["contig", "padded", "offset"])
def test_row_seams(dtype, layout):
    """C at one, exactly full and one-past strides of 64 lanes x one 16-byte vector (256 fp32 / 512 bf16 elements) plus tails, K in
    1, 3, 5, 8, 16 (above C for the small rows), eight class counts per launch as eight tasks without the chain."""
    rows, refs = seam_rows(dtype)
    for K in (1, 3, 5, 8, 16):
        for half in (0, 1):
            sel = range(half * 8, half * 8 + 8)
            logits = [place(rows[i], dtype, layout) for i in sel]
            parents = [None] * 8
            if (K, half) not in refs:
                refs[(K, half)] = run_ref([rows[i] for i in sel], parents, K, consistency=False)
            check(run_kernel(logits, parents, K, consistency=False), refs[(K, half)], f"seams {layout} K={K} C={[SEAM_C[i] for i in sel]}")


def forest(seed, classes, B):
    """A seeded random forest (class 0 of every task the null, without a parent) and B samples of logits: a third on a consistent path,
    a third with the top-1 of a random task moved off the path, a third with a null top-1 at a random task.  Tasks finest first."""
    g = torch.Generator().manual_seed(seed)
    T = len(classes)
    parents = []
    for t in range(T - 1):
        p = torch.randint(1, classes[t + 1], (classes[t],), generator=g, dtype=torch.int32)
        p[0] = -1
        parents.append(p)
    parents.append(None)
    wanted = torch.zeros(B, T, dtype=torch.int64)
    group = torch.arange(B) % 3
    for b in range(B):
        c = int(torch.randint(1, classes[0], (1,), generator=g))
        for t in range(T):
            wanted[b, t] = c
            if t < T - 1:
                c = int(parents[t][c])
        if group[b] == 1:  # off the path: another non-null class of task t whose parent is not the path's
            t = int(torch.randint(0, T - 1, (1,), generator=g))
            others = [c for c in range(1, classes[t]) if int(parents[t][c]) != int(wanted[b, t + 1])]
            wanted[b, t] = others[int(torch.randint(0, len(others), (1,), generator=g))]
        elif group[b] == 2:
            wanted[b, int(torch.randint(0, T, (1,), generator=g))] = 0
    logits = []
    for t in range(T):
        x = torch.randn(B, classes[t], generator=g)
        x[torch.arange(B), wanted[:, t]] += 8.0
        logits.append(x)
    return logits, parents, group.numpy()


FOREST_C = [600, 130, 65, 9]


@DTYPES
def test_chain_on_a_random_forest_and_its_variants(dtype):
    logits_cpu, parents_cpu, group = forest(7, FOREST_C, 37)
    logits = [place(x.to(dtype).float(), dtype, "padded") for x in logits_cpu]
    parents = [None if p is None else p.cuda() for p in parents_cpu]
    want = run_ref(logits, parents, 5)
    f = want[3]
    assert (f[group == 0] == 0).all() and (f[group == 1] == 2).any(1).all() and (f[group == 2] != 0).any(1).all()
    assert all((group == k).sum() >= 12 for k in range(3)) and all((f == v).any() for v in (0, 1, 2))  # nothing passes vacuously
    got = run_kernel(logits, parents, 5)
    check(got, want, f"forest {dtype}")
    again = run_kernel(logits, parents, 5)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), "two launches on the same input differ"
    # without the consistency pass (no parent tables needed)
    check(run_kernel(logits, [None] * 4, 5, consistency=False), run_ref(logits, [None] * 4, 5, consistency=False), "forest raw")
    raw = run_ref(logits, [None] * 4, 5, consistency=False)
    assert not raw[3].any() and (raw[2] == 5).all()
    # one task without a null class: flagged but kept, and the tasks below it are held against its own top-1
    nulls = [0, None, 0, 0]
    w = run_ref(logits, parents, 5, null_index=nulls)
    assert ((w[3][:, 1] != 0) & (w[2][:, 1] == 5)).any()
    check(run_kernel(logits, parents, 5, null_index=nulls), w, "forest null_index=None")
    # 40-bit ids, the nullified entry included
    id_maps = [(torch.arange(c, dtype=torch.int64) * 3 + (1 << 40) + t).cuda() for t, c in enumerate(FOREST_C)]
    w = run_ref(logits, parents, 5, id_maps=id_maps)
    assert w[0].max() > 1 << 40 and (w[0][:, 0, 0] == 1 << 40).any()
    check(run_kernel(logits, parents, 5, id_maps=id_maps), w, "forest id_map")
    # per-sample k, clamped into [1, K]
    kps = torch.tensor([(1, 3, 5, 8, 0, 16, 2)[b % 7] for b in range(37)], dtype=torch.int32).cuda()
    w = run_ref(logits, parents, 8, k_per_sample=kps)
    assert set(np.unique(w[2])) >= {1, 2, 3, 5, 8}
    check(run_kernel(logits, parents, 8, k_per_sample=kps), w, "forest per-sample k")


@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
def test_samples_per_workgroup(B):
    """Four waves per workgroup, one sample each: fewer samples than waves, exactly one workgroup, one past it, more than two."""
    logits_cpu, parents_cpu, _ = forest(20 + B, [65, 7], B)
    logits = [x.cuda() for x in logits_cpu]
    parents = [None if p is None else p.cuda() for p in parents_cpu]
    check(run_kernel(logits, parents, 3), run_ref(logits, parents, 3), f"B={B}")


@DTYPES
def test_ties_follow_the_stated_order(dtype):
    """Integer-valued logits in [-3, 3] over 513 columns: nearly every value ties, the k best are the first k columns holding the maximum."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (9, 513), generator=g).float()
    y = torch.randint(-3, 4, (9, 4), generator=g).float()
    logits = [place(x, dtype, "offset"), place(y, dtype, "contig")]
    parents = [torch.randint(0, 4, (513,), generator=g, dtype=torch.int32).cuda(), None]
    for K in (5, 16):
        raw = run_ref(logits, [None, None], K, consistency=False)
        assert (np.diff(raw[0][:, 0, :], axis=1) > 0).all() and (raw[1][:, 0, 0] == raw[1][:, 0, K - 1]).all()  # one tie holds all K: ascending indices
        check(run_kernel(logits, [None, None], K, consistency=False), raw, f"ties raw K={K}")
        check(run_kernel(logits, parents, K), run_ref(logits, parents, K), f"ties K={K}")


@DTYPES
def test_non_finite_values(dtype):
    """-inf entries have probability 0 and rank last; a NaN ranks first and makes the row's probabilities NaN; -0 and +0 tie."""
    g = torch.Generator().manual_seed(9)
    x = torch.randn(6, 300, generator=g)
    x[0, 5:290] = float("-inf")
    x[1, :] = float("-inf")
    x[1, 299] = 0.25  # everything but one entry: probability exactly 1, then zeros in index order
    x[2, 17] = float("nan")
    x[3, 0] = float("nan")
    x[3, 299] = float("nan")
    x[3, 100] = float("inf")
    x[4, :] = -0.0
    x[4, 1::2] = 0.0
    x[5, 3] = 80.0  # the rest underflows against it
    logits = [place(x, dtype, "padded")]
    want = run_ref(logits, [None], 8, consistency=False)
    assert np.isnan(want[1][2]).all() and want[0][2, 0, 0] == 17 and want[0][3, 0, :3].tolist() == [0, 299, 100]
    assert want[1][1, 0, 0] == 1.0 and (want[1][1, 0, 1:] == 0.0).all() and want[0][1, 0, :3].tolist() == [299, 0, 1]
    assert want[0][4, 0].tolist() == list(range(8))
    check(run_kernel(logits, [None], 8, consistency=False), want, f"non-finite {dtype}")


def test_fixture_of_the_reference():
    """The reference's own results (tests/golden/predict.npz) through DevicePredictor: taxon ids, per-sample k, the (null, 1.0) entries."""
    g = np.load(os.path.join(GOLDEN, "predict.npz"))
    keys = [str(k) for k in g["task_keys"]]
    classes = [int(c) for c in g["num_classes"]]
    p = DevicePredictor(keys, classes, parent_index={k: g[f"parent_{k}"] for k in keys[:-1]}, idx_to_taxon_id={k: g[f"taxon_id_{k}"] for k in keys})
    outputs = {k: torch.from_numpy(g[f"logits_{k}"]).cuda() for k in keys}
    pred = p.predict_logits(outputs, top_k=g["k"].tolist())
    torch.cuda.synchronize()
    ids, probs, count = (pred[n].cpu().numpy() for n in ("ids", "probs", "count"))
    assert np.array_equal(ids, g["ids"]) and np.array_equal(count, g["count"])
    np.testing.assert_allclose(probs, g["probs"], rtol=0, atol=1e-6)
    want = R.predict([g[f"logits_{k}"] for k in keys], [g[f"parent_{k}"] for k in keys[:-1]] + [None], 5, id_maps=[g[f"taxon_id_{k}"] for k in keys],
                     k_per_sample=g["k"])
    check(tuple(pred[n].cpu().numpy() for n in ("ids", "probs", "count", "flags")), want, "fixture")
    res = p.to_results(pred)
    assert len(res) == 24 and [k for k, _ in res[0]] == keys[::-1]
    for b in range(24):
        for t, (key, entries) in enumerate(reversed(res[b])):
            assert key == keys[t] and [i for i, _ in entries] == g["ids"][b, t, : g["count"][b, t]].tolist()
            assert all(isinstance(i, int) and isinstance(pr, float) for i, pr in entries)
    # a per-sample k given as a device tensor is used without a read-back
    k_dev = torch.from_numpy(g["k"]).cuda()  # (the copy from pageable host memory synchronises: made outside the guarded region)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pred16 = p.predict_logits(outputs, top_k=k_dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert pred16["ids"].shape == (24, 4, 16) and np.array_equal(pred16["ids"].cpu().numpy()[:, :, :5], g["ids"])


def test_through_the_model():
    """Eval forward of tests/cases.py's tiny model, bf16 and fp32 compute: predict() = predict_logits(model(...)) bit for bit = the
    reference on the returned logits, and the kernel is handed the plan's own padded rows -- no copy."""
    from linnaeus_amd import build_model
    from oracle import mformer_oracle as O
    from tests.cases import CASES, SEED, make_config, model_state_dict_from_oracle

    spec = CASES["tiny_a"]
    keys = [t for t, _ in spec.heads]
    classes = {t: c for t, c in spec.heads}
    model = build_model(make_config(spec, 64), num_classes=classes)
    model.load_state_dict(model_state_dict_from_oracle(model, O.seeded_state_dict(O.param_shapes(spec), SEED)), strict=True)
    model = model.cuda().eval()
    x, meta = O.seeded_inputs(spec, 9, 64, SEED + 1)
    x, meta = x.cuda(), meta.cuda()
    g = torch.Generator().manual_seed(4)
    parent = torch.randint(1, classes[keys[1]], (classes[keys[0]],), generator=g)
    parent[0] = -1
    p = DevicePredictor(keys, classes, parent_index={keys[0]: parent}, top_k=3)
    seen = {}
    real_forward, real_topk = model.forward, ops.predict_topk

    def forward(*a, **k):
        seen["outputs"] = real_forward(*a, **k)
        return seen["outputs"]

    def topk(logits, *a, **k):
        seen["given"] = [(v.data_ptr(), v.stride(0)) for v in logits]
        return real_topk(logits, *a, **k)

    for dtype in ("fp32", "bf16"):
        model.set_compute_dtype(dtype)
        with torch.no_grad():
            outputs = model(x, meta)
        direct = p.predict_logits(outputs)
        model.forward, ops.predict_topk = forward, topk
        try:
            pred = p.predict(model, x, meta)
        finally:
            del model.forward
            ops.predict_topk = real_topk
        torch.cuda.synchronize()
        for n in ("ids", "probs", "count", "flags"):
            assert pred[n].cpu().numpy().tobytes() == direct[n].cpu().numpy().tobytes(), (dtype, n)
        views = [seen["outputs"][t] for t in p.task_keys]
        assert seen["given"] == [(v.data_ptr(), v.stride(0)) for v in views], "the kernel was not given the forward's own rows"
        assert [v.stride(0) for v in views] == [model._active["logit_ld"][model._active["tasks"].index(t)] for t in p.task_keys]
        assert not model.training and all(v._base is not None for v in views)
        want = run_ref([outputs[t] for t in p.task_keys], [parent.numpy(), None], 3)
        check(tuple(pred[n].cpu().numpy() for n in ("ids", "probs", "count", "flags")), want, f"tiny model {dtype}")
