"""lnx_layernorm_fwd / lnx_layernorm_bwd (csrc/norm.hip) in every lane-group, slot, pair and storage-type instantiation, at every grid
cap and both second stages of the column reduction, against the float64 reference of tests/layernorm_ref.py.

Method.  Every call goes through the C ABI (ops.layernorm_fwd / ops.layernorm_bwd).  lnx_layernorm_fwd_query / _bwd_query say which
instantiation, grid and column-sum route a case runs on: the host-only tests at the top prove that the width tables reach what they
claim, and every GPU case asserts the class it is meant for.  Every output sits in a CANARY-filled buffer (guard rows above and below,
padding columns beyond C, rows a row map skips) that is checked after each call.  Inputs are seeded per case, drawn as in
test_layernorm_fwd_bwd (x = 2 randn + 0.5, w = 1 + 0.2 randn, b = 0.1 randn, dy and gin = randn) and rounded to their storage type
before the reference sees them; the backward takes mean / rstd from the float64 forward reference rounded to fp32, never from the kernel.

Tolerances.  |got - ref| <= rel |ref| + abs against the float64 reference, for inputs at the scale above.  `worst` is the largest
error / bound over this whole file on an MI355X (LNX_LN_RATIOS=<file> makes a run write its own table).
"""
import ctypes
import functools
import json
import os
import zlib

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests import layernorm_ref as R
from tests.data_movement_ref import bits

gpu = pytest.mark.gpu
DT = {L.F32: torch.float32, L.BF16: torch.bfloat16}
NAME = {L.F32: "f32", L.BF16: "bf16"}
EPS = 1e-6
CANARY = -768.0  # exact in bf16 and fp32
NAN = float("nan")

# name: (rel, abs)                                                                                                               worst
TOL = {
    # the project's own bound for an fp32 output (test_layernorm_fwd_bwd): rtol = atol = 2e-5                                      0.019
    "y_f32": (2e-5, 2e-5),
    # one round-to-nearest to an 8-bit significand is 2^-9 |v|; the fp32 value being rounded is within 2e-5 of ref; doubled for a
    # rounding flipped by that difference                                                                                          0.993 (*)
    "y_bf16": (2.0 ** -8, 2e-5),
    # the project's bound for dx in fp32: rtol = atol = 1e-4                                                                       0.003
    "dx_f32": (1e-4, 1e-4),
    # as y_bf16, around a value within 1e-4 of ref (dx2 is rounded from the fp32 product rowscale * dx: the same two terms)       0.984 (*)
    "dx_bf16": (2.0 ** -8, 1e-4),
    # column sums: rel |ref| + abs * sum_m |term| (layernorm_ref's dw_abs / db_abs).  2e-6 ~ 32 fp32 unit round-offs of that sum.  A
    # lane adds at most three rows in sequence at the shapes below; then come <= 4 shuffle steps, 4 waves, and either <= 512 atomics
    # on one address or <= 33 partials per slice in four chains and 64 atomics.  Only the 512-atomic chain is longer than 32 adds, and
    # its partial sums are far smaller than sum |term| (random signs): every shape here stays well inside                         0.046
    "cols": (1e-4, 2e-6),
    # rstd: 1e-5 relative (project).  mean: 1e-5 relative to the row's mean |x| -- a sum's rounding error is relative to the sum of
    # the magnitudes, and at C = 4 a row's mean can cancel to 1e-3 while its terms are ~2                                          0.017
    "stat": (1e-5, 0.0),
}
FP32_OF = {"y_bf16": "y_f32", "dx_bf16": "dx_f32"}
# (*) No head-room, by construction and not by the kernel: the unit round-off of bf16 (8-bit significand) is 2^-8 relative, reached just
# above a power of two (half a step there is 2^-8 of the value; 2^-9 holds only just below the next one), so a correctly rounded
# output touches rel = 2^-8.  within() therefore also asserts the sharp form for bf16 outputs -- got lies between the bf16 roundings of
# ref - t and ref + t, t the fp32 bound of the same quantity -- and the fp32 rows above (same arithmetic, no rounding) show the head-room.
WORST = {}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def within(name, got, ref, extra_abs=None, what=""):
    """|got - ref| <= rel |ref| + abs (x extra_abs, the per-element magnitude, where the bound has one); NaN fails."""
    rel, ab = TOL[name]
    err = (got.double() - ref).abs()
    bound = rel * ref.abs() + (ab if extra_abs is None else ab * extra_abs)
    ratio = float((err / bound).max())
    WORST[name] = max(WORST.get(name, 0.0), ratio)
    print(f"{what} {name}: error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, name, ratio)
    if got.dtype == torch.bfloat16:
        # the sharper statement behind the bf16 bounds (rounding is monotonic): got is the bf16 rounding of SOME value within the
        # fp32 bound of ref.  The bound above cannot tell a correct rounding from an error of one bf16 step just above a power of two.
        t = TOL[FP32_OF[name]][0] * ref.abs() + TOL[FP32_OF[name]][1]
        lo, hi = (ref - t).float().bfloat16(), (ref + t).float().bfloat16()
        n = int(((got < lo) | (got > hi) | got.isnan()).sum())
        assert n == 0, f"{what} {name}: {n} elements are not the rounding of a value within the fp32 bound"


def same_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    n = int((bits(got) != bits(want)).sum())
    assert n == 0, f"{what}: {n} of {got.numel()} elements differ"


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    if os.environ.get("LNX_LN_RATIOS"):
        with open(os.environ["LNX_LN_RATIOS"], "w") as f:
            json.dump(WORST, f, indent=1)


# =====================================================================================================================================
# The tables
# =====================================================================================================================================
SINGLE = [4, 36, 92, 96, 100, 128, 188, 192, 196, 256, 380, 384, 388, 512, 764, 768, 772, 896, 1020, 1024, 1028, 1280, 1532, 1536, 1540,
          1792, 2044, 2048]
PAIR = [8, 40, 88, 96, 104, 128, 184, 192, 200, 256, 376, 384, 392, 512, 760, 768]
# bf16 operands that must run in single mode: (name, C, leading dimension of x or None = C + 8, elements the base of x is moved by)
FALLBACK = [("c_not_8n", 100, None, 0), ("beyond_pair_772", 772, None, 0), ("beyond_pair_1024", 1024, None, 0), ("ldx_100", 96, 100, 0),
            ("base_8_bytes_off", 96, None, 4)]
SINGLE_CLASSES = [(8, 3), (16, 3), (32, 3), (64, 3), (64, 4), (64, 6), (64, 8)]
PAIR_CLASSES = [4, 8, 16, 32]
ONE_PER_CLASS = [36, 96, 128, 192, 256, 384, 512, 768, 896, 1024, 1280, 1536, 1792, 2048]       # single mode: partial and full of each (G, V)
ONE_PER_PAIR_CLASS = [40, 96, 128, 192, 256, 384, 512, 768]
TRIPLES = [(dyd, xd, dxd) for dyd in (L.F32, L.BF16) for xd in (L.F32, L.BF16) for dxd in (L.F32, L.BF16)]
WS_FULL = -1  # a workspace of 2048 * 2 * C floats
# backward caps and slices: name -> (M, C, dw and db wanted, workspace floats or None, grid, route, slices)
CAPS_BWD = {
    "atomics_cap": (512 * 8 + 3, 768, True, None, 512, L.LN_COLS_ATOMICS, 0),
    "no_colsum_cap": (4096 * 8 + 3, 388, False, None, 4096, L.LN_COLS_NONE, 0),
    "workspace_cap": (2048 * 8 + 3, 768, True, WS_FULL, 2048, L.LN_COLS_WORKSPACE, 64),
    "workspace_of_3": (3 * 8 + 5, 768, True, 3 * 2 * 768, 3, L.LN_COLS_WORKSPACE, 1),
    "workspace_too_small": (3 * 8 + 5, 768, True, 2 * 768 - 4, 4, L.LN_COLS_ATOMICS, 0),
    "grid_63": (63 * 64 - 5, 96, True, WS_FULL, 63, L.LN_COLS_WORKSPACE, 1),
    "grid_64": (64 * 64 - 5, 96, True, WS_FULL, 64, L.LN_COLS_WORKSPACE, 64),
    "grid_65": (65 * 64 - 5, 96, True, WS_FULL, 65, L.LN_COLS_WORKSPACE, 64),
}
CAPS_FWD = {"fwd_cap_768": (4096 * 4 + 5, 768, 4096), "fwd_cap_96": (4096 * 32 + 13, 96, 4096)}
MX_PARTIAL = [(37, 512), (37, 640), (21, 896), (21, 1152), (21, 1792)]  # run by test_gpu_ops' two MXFP8 tests


# --- host-only queries: fake, never dereferenced pointers ---------------------------------------------------------------------------
FAKE = 0x10000


def q_fwd(M, C, xd, yd, *, ldx=None, ldy=None, x_off_bytes=0, add=False, ldadd=None, y8=False):
    a, out = L.LnArgs(), L.LnLaunch()
    a.M, a.C, a.eps = M, C, EPS
    a.x, a.x_dtype, a.ldx = FAKE + x_off_bytes, xd, (ldx if ldx is not None else C + 8)
    a.w, a.b, a.y, a.y_dtype, a.ldy = FAKE, FAKE, FAKE, yd, (ldy if ldy is not None else C + 8)
    a.add, a.ldadd = (FAKE if add else None), (ldadd if ldadd is not None else C + 8)
    if y8:
        a.y8, a.y8_scales, a.ldy8 = FAKE, FAKE, C
    rc = L.lib().lnx_layernorm_fwd_query(ctypes.byref(a), ctypes.byref(out))
    return out if rc == 0 else rc


def q_bwd(M, C, dyd, xd, dxd, *, ldx=None, x_off_bytes=0, cols=True, ws_floats=None, ws_off_bytes=0, gin=False, ldgin=None):
    a, out = L.LnBwdArgs(), L.LnLaunch()
    a.M, a.C = M, C
    a.dy, a.dy_dtype, a.lddy = FAKE, dyd, C + 8
    a.x, a.x_dtype, a.ldx = FAKE + x_off_bytes, xd, (ldx if ldx is not None else C + 8)
    a.w, a.mean, a.rstd = FAKE, FAKE, FAKE
    a.dx, a.dx_dtype, a.lddx = FAKE, dxd, C + 8
    a.gin, a.ldgin = (FAKE if gin else None), (ldgin if ldgin is not None else C + 8)
    if cols:
        a.dw, a.db = FAKE, FAKE
    if ws_floats is not None:
        a.ws, a.ws_floats = FAKE + ws_off_bytes, (2048 * 2 * C if ws_floats == WS_FULL else ws_floats)
    rc = L.lib().lnx_layernorm_bwd_query(ctypes.byref(a), ctypes.byref(out))
    return out if rc == 0 else rc


def rows_per_wave(C, pair):
    return 64 // q_fwd(1, C, L.BF16 if pair else L.F32, L.F32).G


def m_of(kind, C, pair):
    """"one": a single row.  "ragged": 11 R - 1 rows = two full workgroups and a rest that ends inside a wave (R > 1) or a workgroup."""
    return 1 if kind == "one" else 11 * rows_per_wave(C, pair) - 1


def test_tables_cover_every_instantiation_and_cap():
    """Host only.  The single table reaches all 14 (G, V, FULL) classes, every partial class at its first and last width and one in
    between; the pair table all 8 (g2, FULL) classes; every fall-back case runs in single mode; every cap case gets the grid, route
    and slice count it is named for; the MXFP8 widths are partial classes of the MXFP8 variant.  Forward and backward agree."""
    cls = {}
    for C in range(4, 2049, 4):
        f, b = q_fwd(77, C, L.F32, L.F32), q_bwd(77, C, L.F32, L.F32, L.F32)
        assert (f.G, f.V, f.pair, f.full, f.mx) == (b.G, b.V, b.pair, b.full, b.mx) and f.pair == 0 and f.mx == 0, C
        assert f.G * f.V * 4 >= C and f.full == (f.G * f.V * 4 == C), C
        cls.setdefault((f.G, f.V, f.full), []).append(C)
    assert sorted(cls) == sorted((g, v, full) for g, v in SINGLE_CLASSES for full in (0, 1))
    for (g, v, full), widths in cls.items():
        hit = [C for C in SINGLE if C in widths]
        if full:
            assert widths == [4 * g * v] and hit == widths, (g, v)
        else:
            assert widths[0] in hit and widths[-1] in hit and any(widths[0] < C < widths[-1] for C in hit), (g, v, hit)
    for C in ONE_PER_CLASS:
        assert C in SINGLE
    assert sorted({k for k, w in cls.items() for C in ONE_PER_CLASS if C in w}) == sorted(cls)

    pcls = set()
    for C in PAIR:
        for yd in (L.BF16, L.F32):
            f, b = q_fwd(77, C, L.BF16, yd), q_bwd(77, C, L.BF16, L.BF16, yd)
            assert (f.G, f.V, f.pair, f.full) == (b.G, b.V, b.pair, b.full) and f.pair == 1 and f.V == 6, C
            assert f.full == (f.G * 24 == C) and f.G * 24 >= C
        pcls.add((f.G, f.full))
        # fp32 x, or fp32 dy with bf16 x, stream through single mode
        assert q_fwd(77, C, L.F32, L.BF16).pair == 0 and q_bwd(77, C, L.F32, L.BF16, L.BF16).pair == 0 and q_bwd(77, C, L.BF16, L.F32, L.BF16).pair == 0
    assert sorted(pcls) == sorted((g, full) for g in PAIR_CLASSES for full in (0, 1))
    assert sorted({(q_fwd(1, C, L.BF16, L.F32).G, q_fwd(1, C, L.BF16, L.F32).full) for C in ONE_PER_PAIR_CLASS}) == sorted(pcls)

    for name, C, ldx, lead in FALLBACK:
        for yd in (L.BF16, L.F32):
            f = q_fwd(77, C, L.BF16, yd, ldx=ldx, x_off_bytes=2 * lead)
            b = q_bwd(77, C, L.BF16, L.BF16, yd, ldx=ldx, x_off_bytes=2 * lead)
            assert f.pair == 0 and b.pair == 0, name
            assert (f.G, f.V) == (b.G, b.V) == (q_fwd(77, C, L.F32, L.F32).G, q_fwd(77, C, L.F32, L.F32).V), name
    assert q_fwd(77, 96, L.BF16, L.BF16).pair == 1 and q_fwd(77, 96, L.BF16, L.BF16, add=True, ldadd=100).pair == 0

    for name, (M, C, cols, ws, grid, route, slices) in CAPS_BWD.items():
        for dxd in (L.F32, L.BF16):
            b = q_bwd(M, C, L.F32, L.F32, dxd, cols=cols, ws_floats=ws)
            assert (b.grid, b.cols, b.slices) == (grid, route, slices), (name, b.grid, b.cols, b.slices)
            if name.endswith("_cap") or name == "workspace_of_3":  # past its cap: the row loop makes a second, ragged trip
                assert b.grid < -(-M // (8 * (64 // b.G))) and M % (8 * (64 // b.G)) != 0, name
    for name, (M, C, grid) in CAPS_FWD.items():
        f = q_fwd(M, C, L.F32, L.F32)
        assert f.grid == grid and grid < -(-M // (4 * (64 // f.G))), name
    for M, C in MX_PARTIAL:
        f = q_fwd(M, C, L.F32, L.BF16, ldy=C, y8=True)
        assert (f.mx, f.full, f.pair) == (1, 0, 0) and f.G == 64, C


def test_misaligned_add_gin_and_workspace_are_refused_on_the_host():
    """ldadd, ldgin (float4 loads) and the workspace base (float4 stores of the partials) are validated before any launch: no GPU is
    touched, the pointers are never dereferenced."""
    lib = L.lib()
    assert q_fwd(8, 96, L.F32, L.F32, add=True, ldadd=98) < 0 and b"ldadd" in lib.lnx_last_error()
    assert q_bwd(8, 96, L.F32, L.F32, L.F32, gin=True, ldgin=98) < 0 and b"ldgin" in lib.lnx_last_error()
    assert q_bwd(8, 96, L.F32, L.F32, L.F32, ws_floats=WS_FULL, ws_off_bytes=8) < 0 and b"16-byte" in lib.lnx_last_error()
    # ... and by the entry points themselves, with their usual message
    a = L.LnArgs()
    a.M, a.C, a.x, a.w, a.b, a.y, a.ldx, a.ldy, a.add, a.ldadd = 8, 96, FAKE, FAKE, FAKE, FAKE, 96, 96, FAKE, 98
    assert lib.lnx_layernorm_fwd(ctypes.byref(a), None) != 0 and b"lnx_layernorm_fwd: ldadd" in lib.lnx_last_error()
    for field, value, msg in (("ldgin", 98, b"lnx_layernorm_bwd: ldgin"), ("ws", FAKE + 8, b"lnx_layernorm_bwd: ws must be 16-byte aligned")):
        g = L.LnBwdArgs()
        g.M, g.C, g.dy, g.x, g.w, g.mean, g.rstd, g.dx, g.lddy, g.ldx, g.lddx = 8, 96, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 96, 96, 96
        g.gin, g.ldgin, g.ws, g.ws_floats = FAKE, 96, FAKE, 2 * 96
        setattr(g, field, value)
        assert lib.lnx_layernorm_bwd(ctypes.byref(g), None) != 0 and msg in lib.lnx_last_error(), field
    # what they accept: a NULL add / gin with any ldadd / ldgin
    assert q_fwd(8, 96, L.F32, L.F32, ldadd=98).grid == 1 and q_bwd(8, 96, L.F32, L.F32, L.F32, ldgin=98).grid == 1


# =====================================================================================================================================
# Guarded buffers
# =====================================================================================================================================
class Guard:
    """`nrows` physical rows of leading dimension ld (default C + 8) inside a CANARY-filled allocation: two guard rows above and
    below, the padding columns [C, ld) of every row, and every row not in `written` stay CANARY.  `.buf` ([nrows, ld]) is what the
    kernel gets; `lead` moves its base by that many elements.  `fill`: a CPU tensor for the written rows, or a constant."""

    def __init__(self, nrows, C, dtype, *, ld=None, written=None, fill=NAN, lead=0, gr=2):
        self.C, self.ld = C, (ld if ld is not None else C + 8)
        assert self.ld >= C
        self.big = torch.full((lead + (nrows + 2 * gr) * self.ld,), CANARY, device="cuda", dtype=dtype)
        lo, hi = lead + gr * self.ld, lead + (gr + nrows) * self.ld
        self.buf = self.big[lo:hi].view(nrows, self.ld)
        self.idx = (torch.arange(nrows) if written is None else written).cuda()
        assert int(self.idx.numel()) == 0 or int(self.idx.max()) < nrows
        self.inside = torch.zeros_like(self.big, dtype=torch.bool)
        if self.idx.numel():
            self.inside[lo:hi].view(nrows, self.ld)[self.idx, :C] = True
            self.buf[self.idx, :C] = fill.cuda().to(dtype) if isinstance(fill, torch.Tensor) else fill

    def check(self, what=""):
        bad = int(((self.big != CANARY) & ~self.inside).sum())  # (a NaN written there counts: NaN != CANARY)
        assert bad == 0, f"{what}: {bad} elements outside the output were written"

    def get(self):
        return self.buf[self.idx, :self.C].cpu()


def vec(n, fill=NAN):
    g = Guard(1, n, torch.float32, fill=fill)
    g.v = g.buf[0, :n]
    return g


def up8(n):
    return (n + 7) // 8 * 8


def workspace(C, floats):
    """A guarded workspace; the library may write its first `floats` floats only."""
    if floats is None:
        return None
    n = 2048 * 2 * C if floats == WS_FULL else floats
    g = Guard(1, n, torch.float32, fill=CANARY)  # (what is written is told from CANARY: the partials never equal it by accident)
    g.v = g.buf[0, :n]
    return g


# =====================================================================================================================================
# Runners
# =====================================================================================================================================
@functools.lru_cache(maxsize=4)
def fwd_inputs(key, M, C, xd, x_map=None, add=False):
    gen = torch.Generator().manual_seed(_seed("fwd", key, M, C, xd, x_map, add))
    nx = int(R.rows(M, x_map).max()) + 1
    x = (2 * torch.randn(nx, C, generator=gen) + 0.5).to(DT[xd])
    w = 1 + 0.2 * torch.randn(C, generator=gen)
    b = 0.1 * torch.randn(C, generator=gen)
    a = torch.randn(M, C, generator=gen).to(DT[xd]) if add else None
    y, mean, rstd = R.forward(x, w, b, EPS, M, C, x_map=x_map, add=a)
    return {"x": x, "w": w, "b": b, "add": a, "y": y, "mean": mean, "rstd": rstd, "absx": x[R.rows(M, x_map)].double().abs().mean(-1)}


def run_fwd(inp, M, C, yd, *, x_map=None, y_map=None, ldx=None, ldy=None, xlead=0, ldadd=None, stats=True, expect=None):
    x = inp["x"]
    X = Guard(x.shape[0], C, x.dtype, ld=ldx, fill=x, lead=xlead)
    yrows = R.rows(M, y_map)
    Y = Guard(int(yrows.max()) + 1, C, DT[yd], ld=ldy, written=yrows)
    W, B = inp["w"].cuda(), inp["b"].cuda()
    A = Guard(M, C, x.dtype, ld=ldadd, fill=inp["add"]) if inp["add"] is not None else None
    MEAN, RSTD = (vec(M), vec(M)) if stats else (None, None)
    kw = dict(M=M, C_=C, ldx=X.ld, ldy=Y.ld, x_map=x_map, y_map=y_map, add=A.buf if A else None, ldadd=A.ld if A else None,
              mean=MEAN.v if stats else None, rstd=RSTD.v if stats else None)
    launch = ops.layernorm_fwd_query(X.buf, W, B, Y.buf, EPS, **kw)
    if expect:
        for k, v in expect.items():
            assert getattr(launch, k) == v, (k, getattr(launch, k), v)
    ops.layernorm_fwd(X.buf, W, B, Y.buf, EPS, **kw)
    torch.cuda.synchronize()
    Y.check("y"), X.check("x")
    out = {"y": Y.get(), "launch": launch}
    if stats:
        MEAN.check("mean"), RSTD.check("rstd")
        out["mean"], out["rstd"] = MEAN.get()[0], RSTD.get()[0]
    return out


def check_fwd(inp, out, yd, what):
    within("y_f32" if yd == L.F32 else "y_bf16", out["y"], inp["y"], what=what)
    if "mean" in out:
        within("stat", out["rstd"], inp["rstd"], what=what + " rstd")
        err = (out["mean"].double() - inp["mean"]).abs() / (TOL["stat"][0] * inp["absx"])
        WORST["stat"] = max(WORST.get("stat", 0.0), float(err.max()))
        assert float(err.max()) <= 1.0, (what, "mean", float(err.max()))


@functools.lru_cache(maxsize=3)
def bwd_inputs(key, M, C, dyd, xd, dy_map=None, x_map=None, relu=False, rowscale=0):
    """CPU operands in storage type and the float64 reference.  relu: x holds exact zeros (a quarter) and negatives.  rowscale = rows
    per sample of a DropPath-like scale with zeros (0 = none)."""
    gen = torch.Generator().manual_seed(_seed("bwd", key, M, C, dyd, xd, dy_map, x_map, relu, rowscale))
    nx, ndy = int(R.rows(M, x_map).max()) + 1, int(R.rows(M, dy_map).max()) + 1
    x = 2 * torch.randn(nx, C, generator=gen) + 0.5
    if relu:
        x[torch.rand(nx, C, generator=gen) < 0.25] = 0.0
    x = x.to(DT[xd])
    w = 1 + 0.2 * torch.randn(C, generator=gen)
    dy = torch.randn(ndy, C, generator=gen).to(DT[dyd])
    gin = torch.randn(nx, C, generator=gen)
    rs = None
    if rowscale:
        rs = (torch.rand(-(-M // rowscale), generator=gen) > 0.3).float() / 0.7
        rs[0] = 0.0
    mean, rstd = R.stats_fp32(x, EPS, M, C, x_map=x_map)
    ref = R.backward(dy, x, w, mean, rstd, M, C, dy_map=dy_map, x_map=x_map, gin=gin, relu_mask=relu, dx2_rowscale=rs, dx2_rows_per_sample=rowscale)
    return {"x": x, "w": w, "dy": dy, "gin": gin, "mean": mean, "rstd": rstd, "rs": rs, "rps": rowscale, "ref": ref}


def run_bwd(inp, M, C, dxd, *, dy_map=None, x_map=None, ldx=None, lddy=None, lddx=None, ldgin=None, xlead=0, gin=True, gin_alias=False, relu=False,
            dw=True, db=True, ws=None, dx2=None, dx2_alias_dy=False, cols_fill=0.0, expect=None):
    x, dy = inp["x"], inp["dy"]
    X = Guard(x.shape[0], C, x.dtype, ld=ldx, fill=x, lead=xlead)
    DY = Guard(dy.shape[0], C, dy.dtype, ld=lddy, fill=dy)
    xrows = R.rows(M, x_map)
    if gin_alias:  # gin and dx are one fp32 buffer: every row holds gin, the mapped rows are overwritten
        assert dxd == L.F32 and gin
        DX = Guard(x.shape[0], C, torch.float32, ld=lddx, fill=inp["gin"])
        GIN = DX
    else:
        DX = Guard(x.shape[0], C, DT[dxd], ld=lddx, written=xrows)
        GIN = Guard(x.shape[0], C, torch.float32, ld=ldgin, fill=inp["gin"]) if gin else None
    W, MEAN, RSTD = inp["w"].cuda(), inp["mean"].cuda(), inp["rstd"].cuda()
    DW, DB = (vec(C, cols_fill) if dw else None), (vec(C, cols_fill) if db else None)
    WS = workspace(C, ws)
    D2 = None
    if dx2_alias_dy:
        D2 = DY
    elif dx2 is not None:
        D2 = Guard(M, C, DT[dx2], ld=up8(C + 8))
    RS = inp["rs"].cuda() if (D2 is not None and inp["rs"] is not None) else None
    kw = dict(M=M, C_=C, lddy=DY.ld, ldx=X.ld, lddx=DX.ld, dy_map=dy_map, x_map=x_map, gin=GIN.buf if GIN else None, ldgin=GIN.ld if GIN else None,
              dw=DW.v if dw else None, db=DB.v if db else None, relu_mask=relu, ws=WS.v if WS else None,
              dx2=D2.buf if D2 else None, lddx2=D2.ld if D2 else None, dx2_rowscale=RS, dx2_rows_per_sample=inp["rps"] if RS is not None else 0)
    launch = ops.layernorm_bwd_query(DY.buf, X.buf, W, MEAN, RSTD, DX.buf, **kw)
    if expect:
        for k, v in expect.items():
            assert getattr(launch, k) == v, (k, getattr(launch, k), v)
    if gin_alias:  # the rows the map skips must keep their gin values: compare them afterwards instead of a canary
        before = DX.buf.clone()
    ops.layernorm_bwd(DY.buf, X.buf, W, MEAN, RSTD, DX.buf, **kw)
    torch.cuda.synchronize()
    X.check("x")
    out = {"launch": launch}
    if gin_alias:
        DX.check("dx (= gin)")
        skipped = torch.ones(x.shape[0], dtype=torch.bool)
        skipped[xrows] = False
        assert torch.equal(DX.buf[skipped.cuda()], before[skipped.cuda()]), "rows the map skips were written"
        out["dx"] = DX.buf[xrows.cuda(), :C].cpu()
    else:
        DX.check("dx")
        out["dx"] = DX.get()
        if GIN:
            GIN.check("gin")
    DY.check("dy")
    if D2 is not None:
        D2.check("dx2")
        out["dx2"] = D2.get()[:M]
    if dw:
        DW.check("dw")
        out["dw"] = DW.get()[0]
    if db:
        DB.check("db")
        out["db"] = DB.get()[0]
    if WS is not None:
        used = launch.grid * 2 * C if launch.cols == L.LN_COLS_WORKSPACE else 0
        WS.inside.zero_()
        WS.inside[2 * WS.ld:2 * WS.ld + used] = True
        WS.check("workspace")
    return out


def check_bwd(inp, out, dxd, what):
    ref = inp["ref"]
    within("dx_f32" if dxd == L.F32 else "dx_bf16", out["dx"], ref["dx"], what=what)
    if "dx2" in out:
        within("dx_f32" if out["dx2"].dtype == torch.float32 else "dx_bf16", out["dx2"], ref["dx2"], what=what + " dx2")
    if "dw" in out:
        within("cols", out["dw"], ref["dw"], ref["dw_abs"], what=what + " dw")
    if "db" in out:
        within("cols", out["db"], ref["db"], ref["db_abs"], what=what + " db")


def width_cases():
    """(id, C, storage type of the streamed inputs, ldx, lead, expected pair mode) of tests 1 and 2."""
    out = [(f"single_{C}", C, L.F32, None, 0, 0) for C in SINGLE]
    out += [(f"pair_{C}", C, L.BF16, None, 0, 1) for C in PAIR]
    out += [(f"fallback_{name}", C, L.BF16, ldx, lead, 0) for name, C, ldx, lead in FALLBACK]
    return [pytest.param(*c[1:], id=c[0]) for c in out]


# =====================================================================================================================================
# 1. Forward at every width
# =====================================================================================================================================
@gpu
@pytest.mark.parametrize("mkind", ["one", "ragged"])
@pytest.mark.parametrize("C,xd,ldx,lead,pair", width_cases())
def test_forward_every_width(C, xd, ldx, lead, pair, mkind):
    M = m_of(mkind, C, pair)
    inp = fwd_inputs("w", M, C, xd)
    for yd in (L.F32, L.BF16):
        what = f"fwd C={C} M={M} {NAME[xd]}->{NAME[yd]}"
        out = run_fwd(inp, M, C, yd, ldx=ldx, xlead=lead, expect={"pair": pair, "mx": 0})
        check_fwd(inp, out, yd, what)
        again = run_fwd(inp, M, C, yd, ldx=ldx, xlead=lead, stats=False)
        same_bits(again["y"], out["y"], what + " without mean / rstd")


# =====================================================================================================================================
# 2. Backward at every width
# =====================================================================================================================================
@gpu
@pytest.mark.parametrize("mkind", ["one", "ragged"])
@pytest.mark.parametrize("C,xd,ldx,lead,pair", width_cases())
def test_backward_every_width(C, xd, ldx, lead, pair, mkind):
    M = m_of(mkind, C, pair)
    inp = bwd_inputs("w", M, C, xd, xd)
    for dxd in (L.F32, L.BF16):
        what = f"bwd C={C} M={M} {NAME[xd]} dx {NAME[dxd]}"
        a = run_bwd(inp, M, C, dxd, ldx=ldx, xlead=lead, expect={"pair": pair, "cols": L.LN_COLS_ATOMICS})
        check_bwd(inp, a, dxd, what + " atomics")
        b = run_bwd(inp, M, C, dxd, ldx=ldx, xlead=lead, ws=WS_FULL, expect={"pair": pair, "cols": L.LN_COLS_WORKSPACE, "slices": 1})
        check_bwd(inp, b, dxd, what + " workspace")
        same_bits(b["dx"], a["dx"], what + " dx workspace vs atomics")
        for dw, db in ((True, False), (False, True), (False, False)):
            c = run_bwd(inp, M, C, dxd, ldx=ldx, xlead=lead, dw=dw, db=db, expect={"pair": pair, "cols": L.LN_COLS_ATOMICS if dw or db else L.LN_COLS_NONE})
            check_bwd(inp, c, dxd, what + f" dw={dw} db={db}")
            same_bits(c["dx"], a["dx"], what + f" dx with dw={dw} db={db}")


@gpu
@pytest.mark.parametrize("dyd,xd,dxd", TRIPLES, ids=[f"{NAME[a]}_{NAME[b]}_{NAME[c]}" for a, b, c in TRIPLES])
@pytest.mark.parametrize("C", [100, 128, 192, 1280, 2048])
def test_backward_every_storage_triple(C, dyd, xd, dxd):
    pair = int(dyd == L.BF16 and xd == L.BF16 and C in (128, 192))
    M = m_of("ragged", C, pair)
    inp = bwd_inputs("t", M, C, dyd, xd)
    what = f"bwd C={C} M={M} {NAME[dyd]}/{NAME[xd]}/{NAME[dxd]}"
    a = run_bwd(inp, M, C, dxd, expect={"pair": pair})
    check_bwd(inp, a, dxd, what)
    b = run_bwd(inp, M, C, dxd, ws=WS_FULL, expect={"pair": pair, "cols": L.LN_COLS_WORKSPACE})
    check_bwd(inp, b, dxd, what + " workspace")
    same_bits(b["dx"], a["dx"], what)


# =====================================================================================================================================
# 3. Options
# =====================================================================================================================================
HW, E, B = 5, 2, 3
N = HW + E
OPTION_WIDTHS = [pytest.param(C, L.F32, 0, id=f"single_{C}") for C in (36, 96, 128, 384, 1280, 2048)] + \
                [pytest.param(C, L.BF16, 1, id=f"pair_{C}") for C in (40, 192)]


@gpu
@pytest.mark.parametrize("C,sd,pair", OPTION_WIDTHS)
def test_forward_row_maps_and_add(C, sd, pair):
    """Patch rows of a token buffer (E extra rows per sample) read through x_map and written one row further through y_map, with
    leading dimensions C + 8; then a skip tensor `add` with its own leading dimension."""
    M = B * HW
    x_map, y_map = (HW, E, E), (HW, E, 1)
    assert R.rows(M, x_map).tolist()[:6] == [2, 3, 4, 5, 6, 9] and R.rows(M, y_map).tolist()[:6] == [1, 2, 3, 4, 5, 8]
    inp = fwd_inputs("map", M, C, sd, x_map)
    for yd in (L.F32, L.BF16):
        out = run_fwd(inp, M, C, yd, x_map=x_map, y_map=y_map, expect={"pair": pair})
        check_fwd(inp, out, yd, f"fwd maps C={C} {NAME[sd]}->{NAME[yd]}")
    for M2 in (M, 1):
        inp = fwd_inputs("add", M2, C, sd, None, True)
        for yd in (L.F32, L.BF16):
            out = run_fwd(inp, M2, C, yd, ldadd=C + 8, expect={"pair": pair})
            check_fwd(inp, out, yd, f"fwd add C={C} M={M2} {NAME[sd]}->{NAME[yd]}")
    # the CLS rows with add, written into row 1 of every sample (the metadata-token form)
    inp = fwd_inputs("cls", B, C, sd, (1, N - 1, 0), True)
    out = run_fwd(inp, B, C, L.F32, x_map=(1, N - 1, 0), y_map=(1, N - 1, 1), ldadd=C + 8, expect={"pair": pair})
    check_fwd(inp, out, L.F32, f"fwd cls + add C={C}")


@gpu
@pytest.mark.parametrize("C,sd,pair", OPTION_WIDTHS)
def test_backward_row_maps_and_gin(C, sd, pair):
    """dy and x through row maps of their own, gin read and dx written through x_map with leading dimensions C + 8; gin aliasing dx
    gives the bits of the out-of-place call and leaves the rows the map skips alone."""
    for name, M, dy_map, x_map in (("cls_x", B, None, (1, N - 1, 0)), ("cls_both", B, (1, N - 1, 0), (1, N - 1, 1)),
                                   ("patch_rows", B * HW, (HW, E, E), (HW, E, 1))):
        inp = bwd_inputs("map", M, C, sd, sd, dy_map, x_map)
        for dxd in (L.F32, L.BF16):
            what = f"bwd maps {name} C={C} {NAME[sd]} dx {NAME[dxd]}"
            out = run_bwd(inp, M, C, dxd, dy_map=dy_map, x_map=x_map, ws=WS_FULL, expect={"pair": pair})
            check_bwd(inp, out, dxd, what)
            if dxd == L.F32:
                alias = run_bwd(inp, M, C, dxd, dy_map=dy_map, x_map=x_map, ws=WS_FULL, gin_alias=True, expect={"pair": pair})
                for k in ("dx", "dw", "db"):
                    same_bits(alias[k], out[k], what + f" gin aliasing dx: {k}")
    M = m_of("ragged", C, pair)
    inp = bwd_inputs("alias", M, C, sd, sd)
    out = run_bwd(inp, M, C, L.F32)
    alias = run_bwd(inp, M, C, L.F32, gin_alias=True)
    same_bits(alias["dx"], out["dx"], f"gin aliasing dx C={C} M={M}")


@gpu
@pytest.mark.parametrize("dyd,xd,dxd", [(L.F32, L.BF16, L.BF16), (L.BF16, L.BF16, L.BF16), (L.F32, L.F32, L.F32)], ids=["f32_bf16_bf16", "bf16", "f32"])
@pytest.mark.parametrize("C", [36, 96, 128, 384, 1280, 2048, 40, 192])
def test_backward_relu_mask(C, dyd, xd, dxd):
    """x is a ReLU output (exact zeros) or negative: those elements of dx are exactly zero, the rest is the plain gradient."""
    M = m_of("ragged", C, 0)
    inp = bwd_inputs("relu", M, C, dyd, xd, None, None, True)
    out = run_bwd(inp, M, C, dxd, relu=True, ws=WS_FULL)
    check_bwd(inp, out, dxd, f"relu C={C} {NAME[dyd]}/{NAME[xd]}/{NAME[dxd]}")
    dead = ~(inp["x"][:M].float() > 0)
    assert int(dead.sum()) > M * C // 8 and int((inp["x"][:M].float() < 0).sum()) > 0
    assert int((bits(out["dx"])[dead] != 0).sum()) == 0, "a masked element of dx is not +0"


@gpu
@pytest.mark.parametrize("C,sd,pair", OPTION_WIDTHS)
def test_backward_second_output(C, sd, pair):
    """dx2 = dx2_rowscale[m / rows_per_sample] * dx in fp32 and bf16, the rowscale holding zeros; dx and the column sums are what they
    are without it; aliasing dy (same type and leading dimension, identity dy_map) changes nothing."""
    M = m_of("ragged", C, pair)
    rps = 4
    inp = bwd_inputs("dx2", M, C, sd, sd, None, None, False, rps)
    ld = up8(C + 8)  # a bf16 dx2 wants 16-byte aligned rows
    for dxd in (L.F32, L.BF16):
        what = f"dx2 C={C} M={M} {NAME[sd]} dx {NAME[dxd]}"
        base = run_bwd(inp, M, C, dxd, lddy=ld, ws=WS_FULL, expect={"pair": pair})
        for d2 in (L.F32, L.BF16):
            out = run_bwd(inp, M, C, dxd, lddy=ld, ws=WS_FULL, dx2=d2, expect={"pair": pair})
            check_bwd(inp, out, dxd, what + f" dx2 {NAME[d2]}")
            for k in ("dx", "dw", "db"):
                same_bits(out[k], base[k], what + f": {k} with dx2")
            assert int((out["dx2"][:rps] != 0).sum()) == 0  # rowscale[0] == 0
            if DT[d2] == inp["dy"].dtype:
                alias = run_bwd(inp, M, C, dxd, lddy=ld, ws=WS_FULL, dx2_alias_dy=True, expect={"pair": pair})
                for k in ("dx", "dx2", "dw", "db"):
                    same_bits(alias[k], out[k], what + f": {k} with dx2 aliasing dy")


# =====================================================================================================================================
# 5. Caps and slices
# =====================================================================================================================================
@gpu
@pytest.mark.parametrize("name", list(CAPS_FWD))
def test_forward_grid_cap(name):
    M, C, grid = CAPS_FWD[name]
    inp = fwd_inputs("cap", M, C, L.F32)
    out = run_fwd(inp, M, C, L.F32, expect={"grid": grid})
    check_fwd(inp, out, L.F32, name)


@gpu
@pytest.mark.parametrize("name", list(CAPS_BWD))
def test_backward_caps_and_slices(name):
    M, C, cols, ws, grid, route, slices = CAPS_BWD[name]
    inp = bwd_inputs("cap", M, C, L.F32, L.F32)
    out = run_bwd(inp, M, C, L.F32, dw=cols, db=cols, ws=ws, expect={"grid": grid, "cols": route, "slices": slices})
    check_bwd(inp, out, L.F32, name)
    if name == "workspace_too_small":  # ... as without a workspace
        plain = run_bwd(inp, M, C, L.F32)
        same_bits(out["dx"], plain["dx"], name)
        for k in ("dw", "db"):
            within("cols", out[k], plain[k].double(), inp["ref"][k + "_abs"], what=name + " vs no workspace")


# =====================================================================================================================================
# 6. Every row counted exactly once
# =====================================================================================================================================
def integer_inputs(M, C, sd):
    """x rows of balanced +-1 with mean = 0 and rstd = 1 passed in (xhat = +-1 exactly), integer dy in [-8, 8], w = 1: every product and
    every partial sum of dw = sum +-dy and db = sum dy is an integer below 2^24, exact in fp32 in any order."""
    gen = torch.Generator().manual_seed(_seed("int", M, C))
    sign = torch.ones(M, C)
    sign[torch.rand(M, C, generator=gen).argsort(-1) < C // 2] = -1.0
    dy = torch.randint(-8, 9, (M, C), generator=gen).float()
    assert C % 2 == 0 and float(sign.sum(-1).abs().max()) == 0 and 8 * M < 2 ** 24
    return {"x": sign.to(DT[sd]), "dy": dy.to(DT[sd]), "w": torch.ones(C), "gin": None, "mean": torch.zeros(M), "rstd": torch.ones(M), "rs": None, "rps": 0,
            "dw": (dy * sign).sum(0), "db": dy.sum(0)}


def exact_colsums(M, C, sd, ws, expect, what):
    inp = integer_inputs(M, C, sd)
    out = run_bwd(inp, M, C, L.F32, gin=False, ws=ws, cols_fill=5.0, expect=expect)  # (dw / db accumulate: they start at 5)
    same_bits(out["dw"], inp["dw"] + 5.0, what + " dw")
    same_bits(out["db"], inp["db"] + 5.0, what + " db")


@gpu
@pytest.mark.parametrize("name", [n for n in CAPS_BWD if CAPS_BWD[n][2]])
def test_exact_column_sums_at_caps_and_slices(name):
    M, C, _, ws, grid, route, slices = CAPS_BWD[name]
    exact_colsums(M, C, L.F32, ws, {"grid": grid, "cols": route, "slices": slices}, name)


@gpu
@pytest.mark.parametrize("C,sd,pair", [pytest.param(C, L.F32, 0, id=f"single_{C}") for C in ONE_PER_CLASS] +
                         [pytest.param(C, L.BF16, 1, id=f"pair_{C}") for C in ONE_PER_PAIR_CLASS])
def test_exact_column_sums_every_class(C, sd, pair):
    M = m_of("ragged", C, pair)
    exact_colsums(M, C, sd, None, {"pair": pair, "cols": L.LN_COLS_ATOMICS}, f"C={C} M={M} atomics")
    exact_colsums(M, C, sd, WS_FULL, {"pair": pair, "cols": L.LN_COLS_WORKSPACE}, f"C={C} M={M} workspace")


# =====================================================================================================================================
# 7. Position independence
# =====================================================================================================================================
@gpu
@pytest.mark.parametrize("sd", [L.F32, L.BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [36, 100, 192, 772, 2048])
def test_a_row_does_not_depend_on_its_position(C, sd):
    """A row's y and dx depend on the row and on C: not on M, on the row's index, or on which lanes beside it are clamped."""
    pair = int(sd == L.BF16 and C == 192)
    M = max(m_of("ragged", C, pair), 4)
    fi = fwd_inputs("pos", M, C, sd)
    bi = bwd_inputs("pos", M, C, sd, sd)

    def part(d, sl):
        return {k: (v[sl].contiguous() if k in ("x", "dy", "gin", "mean", "rstd") else v) for k, v in d.items()}

    for yd in (L.F32, L.BF16):
        whole = run_fwd(fi, M, C, yd, expect={"pair": pair})["y"]
        same_bits(run_fwd(part(fi, slice(0, 1)), 1, C, yd)["y"], whole[:1], f"fwd C={C}: first row alone")
        same_bits(run_fwd(part(fi, slice(M - 3, M)), 3, C, yd)["y"], whole[M - 3:], f"fwd C={C}: last rows in front")
        whole = run_bwd(bi, M, C, yd, expect={"pair": pair})["dx"]
        same_bits(run_bwd(part(bi, slice(0, 1)), 1, C, yd)["dx"], whole[:1], f"bwd C={C}: first row alone")
        same_bits(run_bwd(part(bi, slice(M - 3, M)), 3, C, yd)["dx"], whole[M - 3:], f"bwd C={C}: last rows in front")
