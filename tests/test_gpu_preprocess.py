"""lnx_preprocess / DevicePreprocessor on the MI355X against Pillow's recorded results (tests/golden/preprocess.npz) and the numpy
restatement tests/preprocess_ref.py, which test_preprocess.py holds against Pillow itself.

Everything is compared by exact equality: the fp32 results by their bit patterns, the resized bytes through a second call with
mean = 0 and std = fp32(1 / 255), whose result lies within 1e-4 of the byte and is rounded to it.  The cases take every path of the
kernels: both passes, one pass, neither; windows clipped at both edges; tap counts above the staged chunk of 64 in both passes (573
and 287 horizontal taps at 1000 -> 7, 153 and 77 vertical ones at 301 -> 8); column and row tiles that end inside a tile (224 = 3.5 x 64
columns, 16 / 24 / 7 / 3 columns; 5 / 3 / 4 rows); bicubic overshoot into both clamps (the checkerboards)."""
import io
import os

import numpy as np
import pytest
import torch

from linnaeus_amd import DevicePredictor, DevicePreprocessor
from tests import preprocess_ref as R
from tests.test_preprocess import ALL, GOLDEN, bits, check_against_fixture

pytestmark = pytest.mark.gpu
GUARD = 4096
FILTER = pytest.mark.parametrize("fname", ["bilinear", "bicubic", "nearest"])
_cache = {}


def fixture():
    if "g" not in _cache:
        g = np.load(GOLDEN)
        _cache["g"] = (g, [float(v) for v in g["mean"]], [float(v) for v in g["std"]])
    return _cache["g"]


def source(src, content):
    key = ("src", src, content)
    if key not in _cache:
        _cache[key] = R.pattern(*src, content)
    return _cache[key]


def ref_u8(src, dst, content, fname):
    """The restatement's resized bytes: computed once, shared by every test, never written to."""
    key = ("u8", src, dst, content, fname)
    if key not in _cache:
        _cache[key] = R.resize(source(src, content), dst[0], dst[1], R.FILTERS[fname])
        _cache[key].setflags(write=False)
    return _cache[key]


def preprocessor(dst, fname, mean, std):
    key = ("pre", dst, fname, tuple(mean), tuple(std))
    if key not in _cache:
        _cache[key] = DevicePreprocessor((3,) + tuple(dst), mean, std, fname)
    return _cache[key]


def run(pre, images):
    out = pre(images)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def as_bytes(pre_dst, fname, images):
    """The resized bytes [N, H, W, 3] through the mean = 0, std = 1 / 255 call."""
    x = run(preprocessor(pre_dst, fname, (0.0, 0.0, 0.0), (1 / 255,) * 3), images)
    r = np.rint(x)
    assert np.abs(x - r).max() < 1e-4 and r.min() >= 0 and r.max() <= 255
    return r.astype(np.uint8).transpose(0, 2, 3, 1)


@FILTER
def test_every_case_equals_pillow_and_the_restatement(fname):
    g, mean, std = fixture()
    for src, dst, content in ALL:
        img = source(src, content)
        want = ref_u8(src, dst, content, fname)
        got_u8 = as_bytes(dst, fname, [img])[0]
        assert np.array_equal(got_u8, want), (src, dst, content, fname, np.argwhere(got_u8 != want)[:4].tolist())
        check_against_fixture(g, got_u8, src, dst, content, fname)
        got = run(preprocessor(dst, fname, mean, std), [img])[0]
        assert np.array_equal(bits(got), bits(R.normalize(want, mean, std))), (src, dst, content, fname)
        if (src, dst) not in R.LARGE:
            assert np.array_equal(bits(got), bits(g[f"f32_{R.case_name(src, dst, content)}_{fname}"])), (src, dst, content, fname)


def test_every_byte_value_in_every_channel():
    """A 1 x 256 image at its own size (neither pass runs) through a non-trivial mean / std: the recorded torch CPU result, bit for bit."""
    g, mean, std = fixture()
    every = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    for fname in ("bilinear", "nearest"):
        got = run(preprocessor((1, 256), fname, mean, std), [every])
        assert np.array_equal(bits(got[0, :, 0, :]), bits(g["bytes_f32"])), fname


def mixed_sources():
    """Every case's source in both contents, plus one image that needs no pass at (16, 24) and one that needs only the vertical one."""
    srcs = [source(src, content) for src, _, content in ALL]
    return srcs + [R.pattern(16, 24, "noise"), R.pattern(50, 24, "noise")]


@FILTER
def test_mixed_batch_equals_single_calls_in_any_order(fname):
    _, mean, std = fixture()
    dst = (16, 24)
    pre = preprocessor(dst, fname, mean, std)
    srcs = mixed_sources()
    key = ("mixed", fname)
    if key not in _cache:
        _cache[key] = R.preprocess(srcs, dst[0], dst[1], R.FILTERS[fname], mean, std)
    want = _cache[key]
    single = np.concatenate([run(pre, [s]) for s in srcs])
    assert np.array_equal(bits(single), bits(want)), np.argwhere(bits(single) != bits(want))[:4].tolist()
    batch = run(pre, srcs)
    assert batch.shape == (len(srcs), 3) + dst and np.array_equal(bits(batch), bits(single))
    assert np.array_equal(bits(run(pre, srcs[::-1])), bits(single[::-1]))


@FILTER
def test_guard_regions_stay_untouched(fname):
    """Output and scratch between sentinel regions: the kernels write what they own and nothing else.  The scratch is handed over at
    exactly the size the library asks for."""
    from linnaeus_amd import ops

    _, mean, std = fixture()
    dst = (16, 24)
    pre = DevicePreprocessor((3,) + dst, mean, std, fname)
    srcs = mixed_sources()
    want = run(pre, srcs)
    need = pre.scratch_bytes
    assert (need > 0) == (fname != "nearest")
    sbuf = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    pre._scratch = sbuf[GUARD: GUARD + need] if need else None
    n = len(srcs)
    obuf = torch.full((n * 3 * dst[0] * dst[1] + 2 * GUARD,), -77.0, dtype=torch.float32, device="cuda")
    seen = {}
    real = ops.preprocess_images

    def into_guarded(blob, nbytes, images, off, n_, H, W, code, mean_, std_, scratch, out):
        seen["scratch"] = None if scratch is None else scratch.data_ptr()
        view = obuf[GUARD: GUARD + out.numel()].view(out.shape)
        real(blob, nbytes, images, off, n_, H, W, code, mean_, std_, scratch, view)
        return out

    ops.preprocess_images = into_guarded
    try:
        pre(srcs)
    finally:
        ops.preprocess_images = real
    torch.cuda.synchronize()
    assert seen["scratch"] == (sbuf.data_ptr() + GUARD if need else None)
    got = obuf[GUARD:-GUARD].view(n, 3, *dst).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    assert bool((obuf[:GUARD] == -77.0).all()) and bool((obuf[-GUARD:] == -77.0).all()), "output guards were written"
    assert bool((sbuf[:GUARD] == 0xA5).all()) and bool((sbuf[-GUARD:] == 0xA5).all()), "scratch guards were written"


def test_non_default_stream_and_back_to_back_calls():
    """Three different batches issued without a synchronisation in between, on a side stream: the second reuses nothing of the first
    (the other staging buffer), the third reuses the first's staging buffer, and all share the device buffers."""
    _, mean, std = fixture()
    dst = (16, 24)
    srcs = mixed_sources()
    batches = [srcs[:9], srcs[9:20][::-1], srcs[5:]]
    want = [R.preprocess(b, dst[0], dst[1], R.BICUBIC, mean, std) for b in batches]
    pre = DevicePreprocessor((3,) + dst, mean, std, "bicubic")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        outs = [pre(b) for b in batches]
    stream.synchronize()
    for o, w in zip(outs, want):
        assert np.array_equal(bits(o.cpu().numpy()), bits(w))
    assert pre._pinned[0] is not None and pre._pinned[1] is not None and pre._pinned[0].data_ptr() != pre._pinned[1].data_ptr()
    assert pre._pinned[0].is_pinned() and pre._pinned[1].is_pinned()
    # and again on the default stream, behind the side stream's work
    assert np.array_equal(bits(run(pre, batches[1])), bits(want[1]))


def test_empty_list_and_the_other_input_forms():
    _, mean, std = fixture()
    pre = preprocessor((16, 24), "bilinear", mean, std)
    empty = pre([])
    assert empty.shape == (0, 3, 16, 24) and empty.dtype == torch.float32 and empty.is_cuda
    img = source((37, 53), "noise")
    want = run(pre, [img])
    assert np.array_equal(bits(run(pre, [torch.from_numpy(img.copy())])), bits(want))
    assert np.array_equal(bits(run(pre, [np.asfortranarray(img)])), bits(want))  # any strides
    Image = pytest.importorskip("PIL.Image")
    pil = Image.fromarray(img, "RGB")
    buf = io.BytesIO()
    pil.save(buf, format="PNG")
    both = run(pre, [pil, buf.getvalue()])
    assert np.array_equal(bits(both[0:1]), bits(want)) and np.array_equal(bits(both[1:2]), bits(want))
    grey = Image.fromarray(img[:, :, 0], "L")  # converted as the reference does
    assert np.array_equal(bits(run(pre, [grey])), bits(run(pre, [np.repeat(img[:, :, :1], 3, axis=2)])))


def test_in_front_of_the_predictor():
    """dp.predict(model, pre(images), aux) on tests/cases.py's tiny model = dp.predict on the tensor the restatement builds, exactly."""
    from linnaeus_amd import build_model
    from oracle import mformer_oracle as O
    from tests.cases import CASES, SEED, make_config, model_state_dict_from_oracle

    _, mean, std = fixture()
    spec = CASES["tiny_a"]
    keys = [t for t, _ in spec.heads]
    classes = {t: c for t, c in spec.heads}
    model = build_model(make_config(spec, 64), num_classes=classes)
    model.load_state_dict(model_state_dict_from_oracle(model, O.seeded_state_dict(O.param_shapes(spec), SEED)), strict=True)
    model = model.cuda().eval()
    srcs = mixed_sources()[:9]
    _, meta = O.seeded_inputs(spec, len(srcs), 64, SEED + 1)
    meta = meta.cuda()
    pre = DevicePreprocessor((3, 64, 64), mean, std, "bilinear")
    dp = DevicePredictor(keys, classes, top_k=3, consistency=False)
    want_x = torch.from_numpy(R.preprocess(srcs, 64, 64, R.BILINEAR, mean, std)).cuda()
    pred = dp.predict(model, pre(srcs), meta)
    want = dp.predict(model, want_x, meta)
    torch.cuda.synchronize()
    for n in ("ids", "probs", "count", "flags"):
        assert pred[n].cpu().numpy().tobytes() == want[n].cpu().numpy().tobytes(), n
