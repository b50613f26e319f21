"""The depthwise 7x7 kernels (csrc/dwconv.hip: VALU, csrc/dwconv_mfma.hip: matrix cores) where their software pipeline actually runs:
multi-tile walks, tile-row and image rollovers of the tile cursor, short last walks, padded weight-gradient grids, every seam of the
three tile grids, every compiled dtype variant, through ops.dwconv7 / ops.dwconv7_wgrad against the plain fp64 restatement
tests/dwconv_ref.py (computed on the device from the same, for the bf16 routes bf16-rounded, operands).

Walk arithmetic (restated in tests/dwconv_ref.py, asserted per case from lnx_device_cus() and the margin):
 * MFMA forward / data gradient: 14x14 tiles, ntile = B ceil(H/14) ceil(W/14), numbered row-major over (image, tile row, tile column);
   cus = max(8, device CUs - margin); chunks = min(ntile, max(1, cus / (C/32))); per = ceil(ntile / chunks); workgroup i of a channel
   block walks tiles [i per, min(ntile, (i + 1) per)), fetching tile t + 1 during tile t and writing it to LDS after tile t's stores.
 * MFMA weight gradient: 14x28 tiles, groups = C/32, walkers = min(ntile, max(1, cus / groups)), per = ceil(ntile / walkers),
   walkers = ceil(ntile / per); two 16-channel sibling workgroups per (walker, group), grid = 16 ceil(walkers groups / 8) (padded).
 * VALU forward: 8x16 tiles, per = tiles of one image, halved (rounding up) while ceil(ntile / per) C/32 < 768; no margin.  VALU weight
   gradient: min(ntile, 768 / (C/32)) walkers per channel block, walker i takes tiles i, i + walkers, ...
On 256 CUs: margin 0 / 5 give forward walks of 2 (10x56x56x96), 3 (24x28x28x192), 4, 5, 7 (25x28x28x512, last walk 2), 8 / 9, 13 and
weight-gradient walks of 2, 3, 4 / 5, 7 (64x56x56x96: 74 walkers x 3 groups = 222 pairs in a grid of 448); margin 248 leaves 8 slots, so
every case, the seam sweep included, walks whole images (up to 512 tiles).  test_walk_cases_cover_what_they_claim asserts all of it.

Checks with a tolerance use the per-op suite's numbers unchanged: fp32 kernels 2e-5, bf16 output 8e-3, fp32 output from bf16 operands
1e-4 (rtol = atol), weight / bias gradients rtol 1e-4, atol 2e-5 sqrt(B H W).  Checks without one: integer operands (torch.equal with the
integer answer), position independence (image b bit-identical alone, in a batch, under either margin, beside images of 1e3), sentinel
guards around every y / dw / db of every launch in this file (compared bit for bit), and dw / db started from 0.25 (the += contract).

Measured on the MI355X (256 CUs), worst absolute error over the whole module against the fp64 reference of the same operands:
    output (route)                               | walks               | seams               | bound
    y bf16 (MFMA, fp32 or bf16 x)                | 1.56e-02 of 7.9     | 1.56e-02 of 6.0     | 8e-3 (1 + |y|): half a bf16 ulp at |y| >= 4
    y fp32 (MFMA, bf16 x)                        | 9.2e-07             | 7.2e-07             | 1e-4
    dx fp32 in place (MFMA, bf16 dy)             | 1.0e-06             | 8.9e-07             | 1e-4
    dw (MFMA, fp32 or bf16 x, bf16 dy)           | 5.6e-03 of 1.5e+03  | 1.6e-04 of 4.5e+02  | 1e-4 |dw| + 2e-5 sqrt(BHW) (9e-3 at 64x56x56)
    db (MFMA)                                    | 4.2e-04 of 9.9e+02  | 2.1e-05 of 2.9e+02  | as dw
    y / dx fp32 (VALU, fp32)                     | 3.9e-06 / 1.9e-06   | 2.9e-06 / 1.6e-06   | 2e-5
    dw / db (VALU, fp32)                         | 1.0e-03 / 4.2e-04   | 1.8e-04 / 1.5e-04   | as dw
    y fp32 / dx fp32 (VALU, bf16 operands, child)| 1.7e-06 / 1.0e-06   |                     | 1e-4
    dw / db (VALU, bf16 operands, child)         | 9.6e-04 / 6.4e-04   |                     | as dw
    VALU against MFMA, 3x17x30x64                | y fp32 / bf16: 1.9e-03 (one bf16 ulp, bf16 outputs only), dw 3.1e-05, db 7.6e-06
Every integer, position-independence and guard check held exactly.  381 cases (350 in the parent, 31 in the one child process); wall
time of the module on the MI355X: 8.1 s, of which the child process 3.9 s.

Which test sees which single-line, value-only mutation of the kernels (each built into a scratch copy of the library, one run each;
"old" = tests/test_gpu_ops.py::test_dwconv and ::test_dwconv_mfma, all cases):
    mutation (file: line changed)                                               | old      | failing cases of this module
    dwconv_mfma.hip forward: the prefetched tile is never committed to LDS      | 12 pass  | 97: walks_bf16 29, seams 27, exact_on_integers 20,
      (`if (t + 1 < t_end) sa.commit(xt)` -> never)                              |          |     forward_variants 16, position_independence 5
    dwconv_mfma.hip TileCursor::step: h0 reset without `++b` (the tiles of the   | 12 pass  | 83: walks_bf16 24, exact_on_integers 17, seams 16,
      next image are computed from, and stored to, the walk's first image)      |          |     forward_variants 16, wgrad_variants 6, position_independence 4
    dwconv_mfma.hip taps: `ky * 7 + kc` where FLIP with a bf16 output wants     | 12 pass  | 31: exact_on_integers 22, forward_variants 8 (codes 5, 7),
      `48 - ...` (codes 5 and 7, which nothing else launches)                   |          |     the VALU child (VALU against MFMA)
    dwconv_mfma.hip weight gradient: `sd.add_channel_sums(dbs)` dropped from     | 12 pass  | 68: walks_bf16 27, seams 19, exact_on_integers 19,
      the loop (db holds the first tile of each walk only)                      |          |     wgrad_variants 3
    dwconv_mfma.hip weight gradient: `sx.commit(xt)` dropped from the loop (x    | 12 pass  | 71: walks_bf16 27, seams 19, exact_on_integers 19,
      of a walk's first tile against the dy of every later one)                 |          |     wgrad_variants 6
    dwconv.hip forward: `halo_commit` of the prefetched tile dropped from the    | 12 pass  | 14: walks_fp32 6, exact_on_integers 6,
      loop (VALU, stale LDS tile)                                               |          |     position_independence 1, the VALU child (7-tile bf16 walk)
None of the six touches an address, a mask or a bound of a global access except the second, whose accesses stay inside the tensors.
"""
import os
import re
import subprocess
import sys

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests.dwconv_ref import (dwconv7_ref, launch_cus, mfma_fwd_walk, mfma_wgrad_walk, valu_fwd_walk, valu_wgrad_walk, walk_crossings)

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the GPU")]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF16 = torch.float32, torch.bfloat16
BITS = {F32: torch.int32, BF16: torch.int16}
VALU_CHILD = os.environ.get("LNX_DWCONV_VALU") is not None
MFMA_FILE_VAR = "LNX_TEST_DWCONV_MFMA_RESULTS"
MARGINS = [0, 5, 248]

# (B, H, W, C), forward walk > 1 claimed at margin 0 and 5, weight-gradient walk > 1 claimed at margin 0 and 5; at margin 248 both are
# claimed for every case.  Production shapes: sm stage 0 / 1 (56x56x96, 28x28x192), xl (56x56x256, 28x28x512), lg@384 (96x96x192,
# 48x48x384: 96 = 6 x 14 + 12 and 48 = 3 x 14 + 6, partial tiles in both grids).
WALK_CASES = [
    ((10, 56, 56, 96), True, False),
    ((24, 56, 56, 96), True, True),
    ((64, 56, 56, 96), True, True),
    ((24, 28, 28, 192), True, True),
    ((16, 56, 56, 256), True, True),
    ((25, 28, 28, 512), True, True),
    ((4, 96, 96, 192), True, True),
    ((6, 48, 48, 384), True, True),
    ((40, 28, 28, 160), True, True),
    ((3, 30, 57, 32), False, False),
    ((4, 28, 28, 160), False, False),
]
VALU_WALK_SHAPE = (64, 56, 56, 96)  # 1792 8x16 tiles x 3 channel blocks: per stays 7 (forward) and 7 tiles per walker (weight gradient)


def sid(s):
    return "%dx%dx%dx%d" % tuple(s)


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def r16(t):
    return t.bfloat16().float()


def w49_of(w):  # [C, 7, 7] -> [49][C]
    return w.reshape(w.shape[0], 49).t().contiguous()


def set_margin(m):
    L.check(L.lib().lnx_set_cu_margin(m), "lnx_set_cu_margin")


def cus_at(margin):
    return launch_cus(L.lib().lnx_device_cus(), margin)


WORST = {}


def note(key, got, ref):
    err = float((got.double() - ref).abs().max())
    WORST[key] = max(WORST.get(key, 0.0), err)
    print(f"DWERR {key} {err:.3e} of {float(ref.abs().max()):.3e}")
    return err


# ---- launches: every output lives inside a larger sentinel-filled allocation, compared bit for bit after the call ----
def _guarded(n, guard, dtype):
    buf = (torch.randn(n + 2 * guard, device="cuda") * 100).to(dtype)
    return buf, buf[guard:guard + n]


def _untouched(what, buf, n, guard, before):
    after = torch.cat([bits(buf[:guard]), bits(buf[guard + n:])])
    assert torch.equal(after, before), f"{what}: {int((after != before).sum())} guard elements around it were written"


def conv(x, w49, bias, ydtype, *, flip=False, res=None, inplace=False):
    """ops.dwconv7 into a y that has one image of sentinel before and behind it; y starts as NaN (a pixel nobody writes fails every
    comparison), or as a copy of res which the kernel then updates in place (the production data gradient)"""
    B, H, W, C = x.shape
    n, guard = x.numel(), H * W * C
    buf, flat = _guarded(n, guard, ydtype)
    y = flat.view(B, H, W, C)
    if inplace:
        y.copy_(res)
        res = y
    else:
        y.fill_(float("nan"))
    before = torch.cat([bits(buf[:guard]), bits(buf[guard + n:])]).clone()
    ops.dwconv7(x, w49, bias, y, flip=flip, res=res)
    torch.cuda.synchronize()
    _untouched("y", buf, n, guard, before)
    return y


def wgrad(x, dy, *, start=0.25, with_db=True):
    """ops.dwconv7_wgrad into dw [C, 1, 7, 7] / db [C] that start at `start` (the kernels add) with 32 channels of sentinel around them"""
    C = x.shape[-1]
    bw, fw = _guarded(C * 49, 32 * 49, F32)
    bb, fb = _guarded(C, 32, F32)
    dw, db = fw.view(C, 1, 7, 7), fb
    dw.fill_(start)
    db.fill_(start)
    before_w = torch.cat([bits(bw[:32 * 49]), bits(bw[32 * 49 + C * 49:])]).clone()
    before_b = bits(bb).clone()
    ops.dwconv7_wgrad(x, dy, dw, db if with_db else None)
    torch.cuda.synchronize()
    _untouched("dw", bw, C * 49, 32 * 49, before_w)
    if with_db:
        _untouched("db", bb, C, 32, torch.cat([before_b[:32], before_b[32 + C:]]))
    else:
        assert torch.equal(bits(bb), before_b), "db was written although none was passed"
    return dw.reshape(C, 7, 7), (db if with_db else None)


def inputs(shape, seed, integer=False):
    """x, dy, res [B, H, W, C], w [C, 7, 7], bias [C] on the device.  integer: x, dy in {-1, 0, 1}, taps in [-2, 2], bias in [-3, 3], res in
    [-8, 8]: |y| <= 49 * 2 + 3 = 101, |dx| <= 106, |dw|, |db| <= B H W < 2^24, so fp32 accumulation and a bf16 output are both exact"""
    B, H, W, C = shape
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if integer:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen, device="cuda").float()  # noqa: E731
        return ri(-1, 1, B, H, W, C), ri(-1, 1, B, H, W, C), ri(-8, 8, B, H, W, C), ri(-2, 2, C, 7, 7), ri(-3, 3, C)
    rn = lambda *s: torch.randn(*s, generator=gen, device="cuda")  # noqa: E731
    return rn(B, H, W, C), rn(B, H, W, C), rn(B, H, W, C), rn(C, 7, 7) / 7, rn(C)


_REF = {}


def reference(key, x, w, bias, dy):
    """fp64 (y, dx, dw, db) of the last key only (consecutive cases share it: the margins of one shape)"""
    if key not in _REF:
        _REF.clear()
        _REF[key] = dwconv7_ref(x, w, bias, dy)
    return _REF[key]


def close(key, got, ref, tol):
    assert got.shape == ref.shape
    note(key, got, ref)
    torch.testing.assert_close(got.double(), ref, rtol=tol, atol=tol)


def grads_close(key, dw, db, rw, rb, bhw, start):
    note(key + " dw", dw, rw + start)
    torch.testing.assert_close(dw.double(), rw + start, rtol=1e-4, atol=2e-5 * bhw ** 0.5)
    if db is not None:
        note(key + " db", db, rb + start)
        torch.testing.assert_close(db.double(), rb + start, rtol=1e-4, atol=2e-5 * bhw ** 0.5)


def check_fp32(shape, seed, tag):
    """the VALU kernels: forward, data gradient in place (res aliasing y, flipped taps), weight / bias gradient on top of 0.25"""
    x, dy, res, w, bias = inputs(shape, seed)
    y, dx, dw, db = reference(("fp32", shape, seed), x, w, bias, dy)
    w49 = w49_of(w)
    close(f"{tag} valu fwd fp32->fp32", conv(x, w49, bias, F32), y, 2e-5)
    close(f"{tag} valu dgrad fp32->fp32", conv(dy, w49, None, F32, flip=True, res=res, inplace=True), dx + res.double(), 2e-5)
    gw, gb = wgrad(x, dy)
    grads_close(f"{tag} valu wgrad fp32,fp32", gw, gb, dw, db, shape[0] * shape[1] * shape[2], 0.25)


def check_bf16(shape, seed, tag, kind="mfma"):
    """the production routes of plan.cpp: fp32 x -> bf16 y and bf16 x -> fp32 / bf16 y, bf16 dy into the fp32 residual in place, weight
    gradient of fp32 x / bf16 x with bf16 dy.  The reference sees the bf16-rounded x, w and dy."""
    x, dy, res, w, bias = inputs(shape, seed)
    dy = dy.bfloat16()
    if kind == "valu":  # the VALU kernels widen bf16 operands but do not round fp32 ones
        x, w = r16(x), r16(w)
    y, dx, dw, db = reference(("bf16", shape, seed), r16(x), r16(w), bias, dy)
    w49 = w49_of(w)
    y1 = conv(x, w49, bias, BF16)
    close(f"{tag} {kind} fwd fp32->bf16", y1, y, 8e-3)
    assert torch.equal(bits(conv(x.bfloat16(), w49, bias, BF16)), bits(y1)), "bf16 x and fp32 x (rounded in the stager) give different y"
    close(f"{tag} {kind} fwd bf16->fp32", conv(x.bfloat16(), w49, bias, F32), y, 1e-4)
    close(f"{tag} {kind} dgrad bf16->fp32", conv(dy, w49, None, F32, flip=True, res=res, inplace=True), dx + res.double(), 1e-4)
    bhw = shape[0] * shape[1] * shape[2]
    for xin, name in ((x, "fp32,bf16"), (x.bfloat16(), "bf16,bf16")):
        gw, gb = wgrad(xin, dy)
        grads_close(f"{tag} {kind} wgrad {name}", gw, gb, dw, db, bhw, 0.25)


def assert_walks(shape, margin, claim_fwd, claim_wg):
    f, g = mfma_fwd_walk(*shape, cus_at(margin)), mfma_wgrad_walk(*shape, cus_at(margin))
    print(f"DWWALK {sid(shape)} margin {margin}: forward {f}, weight gradient {g}")
    if claim_fwd or margin == 248:
        assert f["per"] > 1, f"{sid(shape)} margin {margin}: a one-tile forward walk on {L.lib().lnx_device_cus()} CUs: {f}"
    if claim_wg or margin == 248:
        assert g["per"] > 1, f"{sid(shape)} margin {margin}: a one-tile weight-gradient walk on {L.lib().lnx_device_cus()} CUs: {g}"


# ---- 2. multi-tile walks for any grid ----
def test_walk_cases_cover_what_they_claim():
    """over all cases and margins, on this device: forward walks of 2, 3 and 7+ tiles, walks across a tile row and across an image, a
    short last walk, a padded weight-gradient grid whose walks are longer than one tile; all five channel counts; the VALU case"""
    fwd, wg = [], []
    for shape, _, _ in WALK_CASES:
        for m in MARGINS:
            f, g = mfma_fwd_walk(*shape, cus_at(m)), mfma_wgrad_walk(*shape, cus_at(m))
            fwd.append((f["per"],) + walk_crossings(f["ntile"], f["per"], f["tiles_h"], f["tiles_w"]))
            wg.append((g["per"], g["pairs"] % 8 != 0) + walk_crossings(g["ntile"], g["per"], g["tiles_h"], g["tiles_w"]))
    pers = {p for p, *_ in fwd}
    assert {2, 3} <= pers and any(7 <= p < 16 for p in pers), sorted(pers)
    assert any(p > 1 and row for p, row, _, _ in fwd) and any(p > 1 and img for p, _, img, _ in fwd) and any(p > 1 and short for p, _, _, short in fwd)
    assert any(p > 1 and padded for p, padded, *_ in wg), "no multi-tile weight gradient on a padded grid"
    assert any(p > 1 and row for p, _, row, _, _ in wg) and any(p > 1 and img for p, _, _, img, _ in wg) and any(p > 1 and short for p, _, _, _, short in wg)
    assert {s[0][3] for s in WALK_CASES} >= {32, 96, 160, 256, 512}
    assert valu_fwd_walk(*VALU_WALK_SHAPE)["per"] >= 2 and valu_wgrad_walk(*VALU_WALK_SHAPE)["per"] >= 2


@pytest.mark.parametrize("case,margin", [(c, m) for c in WALK_CASES for m in MARGINS], ids=lambda v: sid(v[0]) if isinstance(v, tuple) else f"margin{v}")
def test_walks_bf16(case, margin):
    shape, claim_fwd, claim_wg = case
    set_margin(margin)
    try:
        assert_walks(shape, margin, claim_fwd, claim_wg)
        check_bf16(shape, 1000 + shape[0] + shape[3], f"walk {sid(shape)} m{margin}")
    finally:
        set_margin(0)


@pytest.mark.parametrize("shape", [c[0] for c in WALK_CASES], ids=sid)
def test_walks_fp32(shape):
    """the VALU kernels ignore the margin; their multi-tile case is VALU_WALK_SHAPE, the rest walk one or two tiles"""
    if shape == VALU_WALK_SHAPE:
        assert valu_fwd_walk(*shape)["per"] >= 2 and valu_wgrad_walk(*shape)["per"] >= 2
    check_fp32(shape, 2000 + shape[0] + shape[3], f"walk {sid(shape)}")


# ---- 3. tile seams of the 14x14, 14x28 and 8x16 grids ----
SEAM = [1, 2, 3, 6, 7, 8, 13, 14, 15, 16, 17, 27, 28, 29, 33, 57]
ODD = [w for w in SEAM if w % 2]
# thinned cross product: every height with itself, with a rotation of the list (so every width appears twice) and with an odd width
SEAM_CASES = sorted({(2 + (i + j) % 2, h, w, 64) for i, h in enumerate(SEAM) for j, w in enumerate((h, SEAM[(5 * i + 3) % 16], ODD[(3 * i + 1) % len(ODD)]))})
assert {c[1] for c in SEAM_CASES} == set(SEAM) == {c[2] for c in SEAM_CASES} and {c[0] for c in SEAM_CASES} == {2, 3}
assert all(any(c[1] == h and c[2] % 2 for c in SEAM_CASES) for h in SEAM), "a height lost its odd-width case"


@pytest.mark.parametrize("margin", [0, 248], ids=lambda m: f"margin{m}")
@pytest.mark.parametrize("shape", SEAM_CASES, ids=sid)
@pytest.mark.parametrize("route", ["fp32", "bf16"])
def test_seams(route, shape, margin):
    """H and W on, one below and one above every tile edge, and below the 7-tap window; C = 64 so that another channel block lies
    beside every pixel and B = 2 / 3 so that another image follows every seam; all three kernels (forward, in-place data gradient,
    weight / bias gradient), the guards of conv() / wgrad() around every output"""
    set_margin(margin)
    try:
        (check_fp32 if route == "fp32" else check_bf16)(shape, 3000 + 64 * shape[1] + shape[2], f"seam m{margin}")
    finally:
        set_margin(0)


# ---- 4. every compiled dtype variant: lnx_dwconv7_fwd codes 0..7 = 2 x_dtype + y_dtype + 4 flip, lnx_dwconv7_wgrad codes 0..3 ----
VARIANT_SHAPE = (3, 17, 30, 64)  # partial tiles in all three grids; under margin 248 the MFMA kernels walk 9 / 3 tiles
FWD_VARIANTS = [(code, b, r) for code in range(8) for b in (True, False) for r in (True, False)]
WGRAD_VARIANTS = [(code, d) for code in range(4) for d in (True, False)]
BIG_VALU_VARIANTS = [("fwd", 3), ("dgrad", 6), ("wgrad", 3)]


def vid(v):
    return "code%d-%s" % (v[0], "-".join(("bias" if v[1] else "nobias", "res" if v[2] else "nores")) if len(v) == 3 else ("db" if v[1] else "nodb"))


def variant_inputs():
    """operands that are bf16 numbers already, so that the MFMA kernels (which round fp32 x and the taps) and the VALU kernels (which do
    not) compute the same thing and one fp64 reference serves both"""
    x, dy, res, w, bias = inputs(VARIANT_SHAPE, 4000)
    return r16(x), r16(dy), res, r16(w), bias


def run_fwd_variant(v, ops_in):
    code, with_bias, with_res = v
    x, dy, res, w, bias = ops_in
    flip, xd, yd = code >= 4, (BF16 if code & 2 else F32), (BF16 if code & 1 else F32)
    ref = dwconv7_ref(x, w.flip(1, 2) if flip else w, bias if with_bias else None)[0] + (res.double() if with_res else 0.0)
    got = conv(x.to(xd), w49_of(w), bias if with_bias else None, yd, flip=flip, res=res if with_res else None)
    return got, ref, (8e-3 if yd == BF16 else 2e-5 if code in (0, 4) else 1e-4)


def run_wgrad_variant(v, ops_in):
    code, with_db = v
    x, dy, res, w, bias = ops_in
    _, _, rw, rb = dwconv7_ref(x, w, None, dy)
    gw, gb = wgrad(x.to(BF16 if code & 2 else F32), dy.to(BF16 if code & 1 else F32), with_db=with_db)
    return gw, gb, rw, rb


def on_mfma(v):
    """lnx_dwconv7_fwd's routing in a process without LNX_DWCONV_VALU: a bf16 operand, and no residual into a bf16 output"""
    return v[0] not in (0, 4) and not (v[2] and v[0] & 1) if len(v) == 3 else v[0] != 0


@pytest.mark.skipif(VALU_CHILD, reason="this process is the child")
@pytest.mark.parametrize("margin", [0, 248], ids=lambda m: f"margin{m}")
@pytest.mark.parametrize("v", FWD_VARIANTS, ids=vid)
def test_forward_variants(v, margin):
    """codes 0 / 4 run the VALU kernels, the others the MFMA kernels, except a residual into a bf16 output, which goes to the VALU ones"""
    set_margin(margin)
    try:
        got, ref, tol = run_fwd_variant(v, variant_inputs())
        close(f"variant {'mfma' if on_mfma(v) else 'valu'} fwd code {v[0]}", got, ref, tol)
    finally:
        set_margin(0)


@pytest.mark.skipif(VALU_CHILD, reason="this process is the child")
@pytest.mark.parametrize("margin", [0, 248], ids=lambda m: f"margin{m}")
@pytest.mark.parametrize("v", WGRAD_VARIANTS, ids=vid)
def test_wgrad_variants(v, margin):
    set_margin(margin)
    try:
        gw, gb, rw, rb = run_wgrad_variant(v, variant_inputs())
        grads_close(f"variant {'mfma' if on_mfma(v) else 'valu'} wgrad code {v[0]}", gw, gb, rw, rb, 3 * 17 * 30, 0.25)
    finally:
        set_margin(0)


@pytest.mark.skipif(not VALU_CHILD, reason="LNX_DWCONV_VALU is latched per process: run by test_valu_bf16_variants_in_a_child_process")
@pytest.mark.parametrize("v", [v for v in FWD_VARIANTS + WGRAD_VARIANTS if v[0] not in (0, 4)], ids=vid)
def test_valu_child_variant(v):
    """the VALU kernel of a bf16 variant against fp64, and against what the MFMA kernel gave the parent for the same operands"""
    mfma = torch.load(os.environ[MFMA_FILE_VAR])
    if len(v) == 3:
        got, ref, tol = run_fwd_variant(v, variant_inputs())
        close(f"variant valu fwd code {v[0]}", got, ref, tol)
        if on_mfma(v):
            close(f"valu-vs-mfma fwd code {v[0]}", got, mfma[vid(v)].cuda().double(), tol)
    else:
        gw, gb, rw, rb = run_wgrad_variant(v, variant_inputs())
        grads_close(f"variant valu wgrad code {v[0]}", gw, gb, rw, rb, 3 * 17 * 30, 0.25)
        mw, mb = mfma[vid(v)]
        grads_close(f"valu-vs-mfma wgrad code {v[0]}", gw, gb, mw.cuda().double(), None if mb is None else mb.cuda().double(), 3 * 17 * 30, 0.0)


@pytest.mark.skipif(not VALU_CHILD, reason="LNX_DWCONV_VALU is latched per process: run by test_valu_bf16_variants_in_a_child_process")
def test_valu_child_multi_tile_walk():
    """the bf16 VALU variants on walks of 7 tiles (the parent's VALU runs are fp32 only)"""
    assert valu_fwd_walk(*VALU_WALK_SHAPE)["per"] >= 2 and valu_wgrad_walk(*VALU_WALK_SHAPE)["per"] >= 2
    check_bf16(VALU_WALK_SHAPE, 1000 + 64 + 96, f"walk {sid(VALU_WALK_SHAPE)}", kind="valu")


@pytest.mark.skipif(VALU_CHILD, reason="this process is the child")
def test_valu_bf16_variants_in_a_child_process(tmp_path):
    """LNX_DWCONV_VALU=1 sends every bf16 variant to csrc/dwconv.hip: one fresh process runs them, with the MFMA results of the same
    operands from this process in a file"""
    ops_in, mfma = variant_inputs(), {}
    for v in FWD_VARIANTS:
        if on_mfma(v):
            mfma[vid(v)] = run_fwd_variant(v, ops_in)[0].cpu()
    for v in WGRAD_VARIANTS:
        if on_mfma(v):
            gw, gb = run_wgrad_variant(v, ops_in)[:2]
            mfma[vid(v)] = (gw.cpu(), None if gb is None else gb.cpu())  # on top of the same 0.25
    path = str(tmp_path / "mfma_results.pt")
    torch.save(mfma, path)
    want = 24 + 6 + 1
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", __file__, "-q", "-s", "-k", "valu_child", "-p", "no:cacheprovider"], cwd=REPO,
                           env={**os.environ, "LNX_DWCONV_VALU": "1", MFMA_FILE_VAR: path}, timeout=900, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the LNX_DWCONV_VALU child hung; nothing more is started on the GPU\n{e.stdout}", returncode=1)
    print("\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("DWERR")))
    tail = "\n".join(r.stdout.strip().splitlines()[-30:])
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"the LNX_DWCONV_VALU child died (status {r.returncode}); nothing more is started on the GPU\n{tail}\n{r.stderr[-2000:]}", returncode=1)
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) == want and "failed" not in r.stdout.strip().splitlines()[-1], tail


# ---- 5. tests without a tolerance ----
@pytest.mark.skipif(VALU_CHILD, reason="this process is the child")
@pytest.mark.parametrize("case,margin", [(c, m) for c in WALK_CASES for m in (0, 248)], ids=lambda v: sid(v[0]) if isinstance(v, tuple) else f"margin{v}")
def test_exact_on_integers(case, margin):
    """Small-integer operands: every product and every partial sum is an integer below 2^24 (and |y| <= 106 < 256 for a bf16 output), so
    every kernel must return the integer answer exactly.  A swapped kx / ky, a wrong flip, a stale LDS tile, a tile of the wrong image
    or the wrong channel of a wave pair changes an integer."""
    shape = case[0]
    x, dy, res, w, bias = inputs(shape, 5000 + shape[0] + shape[3], integer=True)
    y, dx, dw, db = (t.float() for t in dwconv7_ref(x, w, bias, dy))
    w49 = w49_of(w)
    set_margin(margin)
    try:
        assert_walks(shape, margin, case[1], case[2])
        for xd in (F32, BF16):  # MFMA codes 1, 3, 2, then the flipped 5, 7, 6 (+ residual in place)
            assert torch.equal(conv(x.to(xd), w49, bias, BF16).float(), y), f"forward {xd} -> bf16"
            assert torch.equal(conv(dy.to(xd), w49, None, BF16, flip=True).float(), dx), f"flipped {xd} -> bf16"
        assert torch.equal(conv(x.bfloat16(), w49, bias, F32), y), "forward bf16 -> fp32"
        assert torch.equal(conv(dy.bfloat16(), w49, None, F32, flip=True, res=res, inplace=True), dx + res), "data gradient bf16 -> fp32 in place"
        for xd, dyd in ((F32, BF16), (BF16, F32), (BF16, BF16)):
            gw, gb = wgrad(x.to(xd), dy.to(dyd), start=3.0)
            assert torch.equal(gw, dw + 3.0) and torch.equal(gb, db + 3.0), f"weight gradient {xd}, {dyd}"
        if margin == 0:  # the VALU kernels (no margin)
            assert torch.equal(conv(x, w49, bias, F32), y), "VALU forward"
            assert torch.equal(conv(dy, w49, None, F32, flip=True, res=res, inplace=True), dx + res), "VALU data gradient in place"
            assert torch.equal(conv(dy, w49, bias, BF16, flip=True, res=res).float(), dx + res + bias), "VALU flipped, residual into bf16"
            gw, gb = wgrad(x, dy, start=3.0)
            assert torch.equal(gw, dw + 3.0) and torch.equal(gb, db + 3.0), "VALU weight gradient"
    finally:
        set_margin(0)


@pytest.mark.skipif(VALU_CHILD, reason="this process is the child")
@pytest.mark.parametrize("shape,b", [((3, 30, 57, 32), 1), ((4, 28, 28, 160), 2), ((5, 56, 56, 96), 3), ((3, 17, 29, 64), 0), ((12, 28, 28, 512), 7)], ids=lambda v: sid(v) if isinstance(v, tuple) else f"image{v}")
@pytest.mark.parametrize("route", ["fp32", "bf16"])
def test_position_independence(route, shape, b):
    """Forward and data gradient have no arithmetic across tiles: image b's output is the same bits alone, in the batch, under margin 0
    and 248 (other walks, other workgroups, other prefetch order), and with every other image set to +-1e3"""
    x, dy, res, w, bias = inputs(shape, 6000 + shape[3])
    xd, yd = (F32, F32) if route == "fp32" else (F32, BF16)
    gd = F32 if route == "fp32" else BF16
    w49 = w49_of(w)
    loud_x, loud_dy = x.clone(), dy.clone()
    others = [i for i in range(shape[0]) if i != b]
    sign = torch.where(torch.rand(x[others].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) < 0.5, -1e3, 1e3)
    loud_x[others], loud_dy[others] = sign, -sign

    def run(xs, dys, rs):
        return bits(conv(xs.to(xd), w49, bias, yd)), bits(conv(dys.to(gd), w49, None, F32, flip=True, res=rs, inplace=True))

    try:
        set_margin(0)
        alone = run(x[b:b + 1], dy[b:b + 1], res[b:b + 1])
        alone = (alone[0][0], alone[1][0])
        for margin in (0, 248):
            set_margin(margin)
            for what, (xs, dys) in (("batch", (x, dy)), ("loud neighbours", (loud_x, loud_dy))):
                got = run(xs, dys, res)
                assert torch.equal(got[0][b], alone[0]), f"forward of image {b}: {what}, margin {margin} differs from the image alone"
                assert torch.equal(got[1][b], alone[1]), f"data gradient of image {b}: {what}, margin {margin} differs from the image alone"
                if what == "loud neighbours":
                    assert not torch.equal(got[0][others[0]], alone[0]), "the other images were not replaced"
    finally:
        set_margin(0)
