"""Kernel-level tests of the HBM-bound data-movement kernels (csrc/elementwise.hip: the per-step weight refresh, the dropout passes,
im2col / scale_cast / LayerScale / fill / colsum / aggregate / pack_meta; csrc/collate.hip: the row mixing) against the plain torch
references of tests/data_movement_ref.py.

Method, for every case: seeded random inputs (a shifted or swapped element cannot compare equal by accident); every output sits in
a larger buffer whose surroundings hold CANARY and are checked afterwards; an overwritten output is prefilled with NaN, an
accumulated one with random non-zero values.  Tolerances: copies, casts and single fp32 products are compared BIT FOR BIT; the
rest use the derived bounds of data_movement_ref (fma_bound, blend_bound, summation_bound) and nothing measured."""
import ctypes as C

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests import data_movement_ref as R

pytestmark = pytest.mark.gpu
DT = {L.F32: torch.float32, L.BF16: torch.bfloat16}
BOTH = pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=["f32", "bf16"])
CANARY = -768.0  # exact in bf16 and fp32
NAN = float("nan")


def cgen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def randn(gen, *shape):
    return torch.randn(*shape, generator=gen, device="cuda")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Guarded:
    """A rows x cols window (leading dimension cols + 2 gc) inside a CANARY-filled buffer: gr rows above and below, gc columns left
    and right.  gc is a multiple of 8, so the window keeps the 16-byte alignment of the allocation when cols % 8 == 0."""

    def __init__(self, rows, cols, dtype, fill, gr=2, gc=8):
        self.big = torch.full((rows + 2 * gr, cols + 2 * gc), CANARY, device="cuda", dtype=dtype)
        self.rs, self.cs = slice(gr, gr + rows), slice(gc, gc + cols)
        self.win = self.big[self.rs, self.cs]
        self.win.copy_(fill) if isinstance(fill, torch.Tensor) else self.win.fill_(fill)
        self.ld = self.big.stride(0)

    def assert_canaries(self):
        outside = torch.ones_like(self.big, dtype=torch.bool)
        outside[self.rs, self.cs] = False
        bad = int((self.big[outside] != CANARY).sum())  # (a NaN written there counts: NaN != CANARY)
        assert bad == 0, f"{bad} elements outside the output window were written"


def flat(n, dtype, fill, shape=None):
    """n contiguous elements with 64 canary elements before and after; .win is viewed as `shape`."""
    g = Guarded(1, n, dtype, fill.reshape(1, n) if isinstance(fill, torch.Tensor) else fill, gr=0, gc=64)
    g.win = g.win.reshape(shape if shape is not None else (n,))
    assert g.win.data_ptr() == g.big.data_ptr() + 64 * g.big.element_size()  # a view, not a copy
    return g


def assert_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = R.bits(got) != R.bits(want)
    n = int(bad.sum())
    if n:
        first = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ, the first at {first}: got {got[tuple(first)].item()!r}, want {want[tuple(first)].item()!r}")


def assert_within(got, ref64, bound, what=""):
    """|got - ref64| <= bound element-wise (a NaN in got fails)."""
    err = (got.double() - ref64).abs()
    bad = ~(err <= bound)
    n = int(bad.sum())
    if n:
        first = tuple(torch.nonzero(bad)[0].tolist())
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements outside the bound, the first at {list(first)}: got {got[first].item()!r}, "
                             f"want {ref64[first].item()!r} +- {bound[first].item():.3e}")


# =====================================================================================================================================
# 1. lnx_prep_weights
# =====================================================================================================================================
# One table, launched once per destination type.  (name, mode, rows, cols, ld, P, ld_t or 0, source offset in floats)
PREP_TABLE = [
    # fast path (CAST, ld == cols, 16-byte aligned, rows * cols % 4 == 0), each followed by a tensor of another path so that an
    # off-by-one of the descriptor search shows in the neighbour
    ("fast_2048", L.PREP_CAST, 32, 64, 64, 0, 0, 0),          # exactly one workgroup
    ("scalar_ld", L.PREP_CAST, 5, 48, 64, 0, 0, 0),           # scalar: ld > cols, columns 48..63 zero
    ("fast_2052", L.PREP_CAST, 27, 76, 76, 0, 0, 0),          # one workgroup + 4 elements
    ("scalar_misaligned", L.PREP_CAST, 6, 10, 10, 0, 0, 1),   # scalar: source one float off 16-byte alignment (60 % 4 == 0)
    ("fast_4", L.PREP_CAST, 1, 4, 4, 0, 0, 0),                # one vector
    ("scalar_odd", L.PREP_CAST, 3, 7, 7, 0, 0, 0),            # scalar: rows * ld % 4 != 0
    ("fast_38_blocks", L.PREP_CAST, 300, 256, 256, 0, 0, 0),  # 37.5 workgroups
    ("perm_32", L.PREP_CONV_PERM, 24, 128, 128, 4, 0, 0),     # C = 32, ld == cols
    ("perm_45_ld", L.PREP_CONV_PERM, 10, 180, 192, 4, 0, 0),  # C = 45 (no power of two), ld > cols
    ("t_tiles", L.PREP_CAST, 64, 128, 128, 0, 72, 0),         # transposed copy: 2 x 2 whole tiles of 32 rows x 64 columns
    ("no_t_between", L.PREP_CAST, 7, 12, 12, 0, 0, 0),        # dst_t == NULL between two that have one
    ("t_33x65", L.PREP_CAST, 33, 65, 65, 0, 40, 0),           # one row / one column past a tile in each direction
    ("t_row", L.PREP_CAST, 1, 50, 50, 0, 4, 0),               # rows = 1
    ("t_col", L.PREP_CAST, 50, 1, 1, 0, 56, 0),               # cols = 1
    ("t_perm", L.PREP_CONV_PERM, 40, 80, 88, 4, 48, 0),       # CONV_PERM (C = 20) with a transposed copy and K padding
    ("dw49_32", L.PREP_DW49, 32, 49, 49, 0, 0, 0),
    ("dw49_96", L.PREP_DW49, 96, 49, 49, 0, 0, 0),            # 4704 elements: three workgroups
    ("dw49_45", L.PREP_DW49, 45, 49, 49, 0, 0, 0),            # 2205 elements: no multiple of 256, the workgroup boundary falls mid-tap
]


@BOTH
def test_prep_weights_table(dtype):
    """Every path of prep_weights_kernel in ONE launch: the cast is round-to-nearest-even (= Tensor.to(bfloat16)) or a copy, so
    every destination, its zero K padding, the caller's padding of the transposed copies and the canaries compare bit for bit."""
    tdt = DT[dtype]
    gen = cgen(101 + dtype)
    lib = L.lib()
    descs = (L.PrepDesc * len(PREP_TABLE))()
    keep, blk = [], 0
    for d, (name, mode, rows, cols, ld, P, ld_t, src_off) in zip(descs, PREP_TABLE):
        src = randn(gen, src_off + rows * cols)[src_off:].view(rows, cols)
        assert src.data_ptr() % 16 == 4 * src_off
        if mode == L.PREP_DW49:
            dst, want = flat(49 * rows, torch.float32, NAN), R.prep_dw49(src).reshape(-1)
        else:
            dst, want = flat(rows * ld, tdt, NAN, (rows, ld)), R.prep_main(src, ld, tdt, P)
        dst_t = Guarded(cols, ld_t, tdt, CANARY / 2, gr=2, gc=0) if ld_t else None  # [cols, ld_t]: columns rows..ld_t-1 keep CANARY / 2
        d.src, d.dst, d.dst_t = src.data_ptr(), dst.win.data_ptr(), dst_t.win.data_ptr() if dst_t else None
        d.rows, d.cols, d.ld, d.ld_t, d.P, d.mode, d.block_start = rows, cols, ld, ld_t, P, mode, blk
        blk += lib.lnx_prep_blocks(rows, ld, cols, ld_t, int(dst_t is not None))  # as lnx_plan_bind builds the table
        keep.append((name, src, dst, want, dst_t, P))
    assert blk > len(PREP_TABLE)
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).cuda()
    L.check(lib.lnx_prep_weights(_p(table), len(PREP_TABLE), blk, dtype, _stream()), "lnx_prep_weights")
    torch.cuda.synchronize()
    for name, src, dst, want, dst_t, P in keep:
        assert_bits(dst.win, want, name)
        dst.assert_canaries()
        if dst_t is not None:
            rows = src.shape[0]
            assert_bits(dst_t.win[:, :rows].contiguous(), R.prep_transposed(src, tdt, P), name + " transposed")
            assert bool((dst_t.win[:, rows:] == CANARY / 2).all()), name + ": the padding columns of the transposed copy were written"
            dst_t.assert_canaries()


# =====================================================================================================================================
# 2. lnx_dropout_mul / lnx_dropout_residual
# =====================================================================================================================================
# M * C / 8 below one workgroup; 333 = no multiple of 256 with C / 8 = 9 odd (workgroups straddle rows); 2 107 400 > 8192 * 256 (the
# second trip of the grid-stride loop)
DROP_SHAPES = [(3, 40), (37, 72), (8200, 2056)]
INV_KEEP = float(torch.tensor(1.0 / 0.7, dtype=torch.float32))  # an fp32 value, so that c_float passes it on unchanged


def draw_mask(gen, M, Cc):
    """Keep bytes from {0, 1, 2, 255}: any non-zero byte keeps."""
    vals = torch.tensor([0, 1, 2, 255], dtype=torch.uint8, device="cuda")
    return vals[torch.randint(0, 4, (M, Cc), generator=gen, device="cuda")]


def run_dropout_mul(x, dtype, mask, M, Cc):
    L.check(L.lib().lnx_dropout_mul(_p(x), dtype, _p(mask), C.c_float(INV_KEEP), M, Cc, _stream()), "lnx_dropout_mul")
    torch.cuda.synchronize()


@BOTH
@pytest.mark.parametrize("M,Cc", DROP_SHAPES)
def test_dropout_mul(M, Cc, dtype):
    """Exact: one fp32 product (then one rounding to bf16), or a literal zero."""
    gen = cgen(M + Cc + dtype)
    x0 = randn(gen, M, Cc).to(DT[dtype])
    mask = draw_mask(gen, M, Cc)
    x = flat(M * Cc, DT[dtype], x0.reshape(-1), (M, Cc))
    run_dropout_mul(x.win, dtype, mask, M, Cc)
    assert_bits(x.win, R.dropout_mul(x0, mask, INV_KEEP), "dropout_mul")
    x.assert_canaries()


@BOTH
def test_dropout_mul_drops_non_finite_inputs_to_zero(dtype):
    """include/lnx.h defines a select, not a multiply by 0: a dropped Inf or NaN comes out as exactly +0, a kept one stays."""
    M, Cc = 37, 72
    gen = cgen(7 + dtype)
    x0 = randn(gen, M, Cc)
    mask = draw_mask(gen, M, Cc)
    special = torch.tensor([float("inf"), float("-inf"), NAN], device="cuda")[torch.randint(0, 3, (M, Cc), generator=gen, device="cuda")]
    x0 = torch.where(torch.rand(M, Cc, generator=gen, device="cuda") < 0.5, special, x0).to(DT[dtype])
    dropped = mask == 0
    assert int((dropped & ~torch.isfinite(x0)).sum()) > 100 and int((~dropped & ~torch.isfinite(x0)).sum()) > 100
    x = flat(M * Cc, DT[dtype], x0.reshape(-1), (M, Cc))
    run_dropout_mul(x.win, dtype, mask, M, Cc)
    assert int((R.bits(x.win)[dropped] != 0).sum()) == 0
    want = R.dropout_mul(x0, mask, INV_KEEP)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(x.win), nan)
    assert_bits(torch.where(nan, torch.zeros_like(want), x.win), torch.where(nan, torch.zeros_like(want), want), "dropout_mul, non-finite")
    x.assert_canaries()


@BOTH
@pytest.mark.parametrize("with_rowscale", [False, True], ids=["plain", "rowscale"])
@pytest.mark.parametrize("M,Cc", DROP_SHAPES)
def test_dropout_residual(M, Cc, with_rowscale, dtype):
    """Dropped elements: out == res bit for bit.  Kept: within data_movement_ref.fma_bound of the float64 value (the kernel may or
    may not contract z * rs + res into an fma)."""
    gen = cgen(3 * M + Cc + 2 * dtype + with_rowscale)
    z = randn(gen, M, Cc).to(DT[dtype])
    res = randn(gen, M, Cc)
    mask = draw_mask(gen, M, Cc)
    rps = 7 if M > 7 else 2  # does not divide 3, 37 or 8200
    assert M % rps != 0
    rowscale = None
    if with_rowscale:
        rowscale = 0.5 + torch.rand((M + rps - 1) // rps, generator=gen, device="cuda")
        rowscale[1] = 0.0
    out = flat(M * Cc, torch.float32, NAN, (M, Cc))
    L.check(L.lib().lnx_dropout_residual(_p(z), dtype, _p(mask), C.c_float(INV_KEEP), _p(rowscale), rps if with_rowscale else 0, _p(res), _p(out.win), M, Cc,
                                         _stream()), "lnx_dropout_residual")
    torch.cuda.synchronize()
    ref, bound = R.dropout_residual(z, mask, INV_KEEP, rowscale, rps, res)
    dropped = mask == 0
    assert int((R.bits(out.win)[dropped] != R.bits(res)[dropped]).sum()) == 0, "a dropped element is not the residual bit for bit"
    assert_within(out.win, ref, bound, "dropout_residual")
    out.assert_canaries()


# =====================================================================================================================================
# 3. grid caps, strides and row maps of the remaining entry points
# =====================================================================================================================================
ROW_MAP = (7, 3, 2)  # group, pad, off: all non-zero


def mapped_rows(M):
    return M + (M - 1) // ROW_MAP[0] * ROW_MAP[1] + ROW_MAP[2]  # rows a mapped buffer needs for m in [0, M)


@BOTH
def test_scale_cast_grid_cap_strides_row_map(dtype):
    """M * C / 4 = 1 048 808 > 4096 * 256 vectors: every workgroup takes a second trip.  Exact: one fp32 product, one rounding."""
    M, Cc, rps = 131101, 32, 1000
    assert M * Cc // 4 > 4096 * 256 and M % ROW_MAP[0] != 0 and M % rps != 0
    gen = cgen(31 + dtype)
    src = Guarded(mapped_rows(M), Cc, torch.float32, 0.0)  # ldin = 48 > C
    src.win.copy_(randn(gen, mapped_rows(M), Cc))
    rowscale = 0.5 + torch.rand((M + rps - 1) // rps, generator=gen, device="cuda")
    rowscale[3] = 0.0
    out = Guarded(M, Cc, DT[dtype], NAN)
    ops.scale_cast(src.win, out.win, M, Cc, ldin=src.ld, in_map=ROW_MAP, rowscale=rowscale, rows_per_sample=rps, ldout=out.ld)
    torch.cuda.synchronize()
    want = (src.win[R.map_rows(M, ROW_MAP, "cuda")] * R.row_scale(rowscale, rps, M)).to(DT[dtype])
    assert_bits(out.win, want, "scale_cast")
    out.assert_canaries()


def test_fill_rows_grid_cap_strides_row_map():
    M, Cc = 131101, 32
    gen = cgen(32)
    vec = randn(gen, Cc)
    out = Guarded(mapped_rows(M), Cc, torch.float32, CANARY / 2)  # the rows between the mapped ones must keep their value
    ops.fill_rows(vec, out.win, out.ld, ROW_MAP, M, Cc)
    torch.cuda.synchronize()
    want = torch.full_like(out.win, CANARY / 2)
    want[R.map_rows(M, ROW_MAP, "cuda")] = vec
    assert_bits(out.win, want, "fill_rows")
    out.assert_canaries()


def test_colsum_rows_many_blocks_strides_row_map():
    """94 workgroups of 32 rows (the last of 25), C = 300 > 256 columns (two trips of the column loop), float atomics into a
    non-zero output: the worst-case summation bound over the n rows and the value already there."""
    M, Cc = 3001, 300
    assert M % 32 != 0 and M % ROW_MAP[0] != 0
    gen = cgen(33)
    src = Guarded(mapped_rows(M), Cc, torch.float32, 0.0)
    src.win.copy_(randn(gen, mapped_rows(M), Cc))
    acc0 = randn(gen, Cc)
    acc = flat(Cc, torch.float32, acc0)
    ops.colsum_rows(src.win, src.ld, ROW_MAP, acc.win, M, Cc)
    torch.cuda.synchronize()
    terms = src.win[R.map_rows(M, ROW_MAP, "cuda")].double()
    assert_within(acc.win, acc0.double() + terms.sum(0), R.summation_bound(M, acc0.double().abs() + terms.abs().sum(0)), "colsum_rows")
    acc.assert_canaries()


# C = 4: 256 rows a workgroup; C = 96: C / 4 = 24 does not divide 256 (10 rows, 16 idle lanes); C = 1024: one row a workgroup.
# The small M leaves the last workgroup partly filled; the large one exceeds 2048 workgroups * 8 trips * rows per workgroup, so the
# 2048-workgroup cap makes every workgroup loop on past its 8 trips.
@BOTH
@pytest.mark.parametrize("Cc,M", [(4, 1501), (96, 151), (1024, 19), (4, 2048 * 8 * 256 + 1501), (96, 2048 * 8 * 10 + 151), (1024, 2048 * 8 + 19)])
def test_layerscale_bwd(Cc, M, dtype):
    tdt = DT[dtype]
    rps = 8 if M < 10000 else 4099
    assert M % rps != 0 and M > 2 * rps
    gen = cgen(Cc + M % 1000 + dtype)
    g = randn(gen, M, Cc)
    z = randn(gen, M, Cc).to(tdt)
    gamma = randn(gen, Cc)
    rowscale = 0.5 + torch.rand((M + rps - 1) // rps, generator=gen, device="cuda")
    rowscale[1] = 0.0
    dz = Guarded(M, Cc, tdt, NAN, gr=2, gc=0)
    dg0 = randn(gen, Cc)
    dgamma = flat(Cc, torch.float32, dg0)
    ops.layerscale_bwd(g, z, gamma, rowscale, rps, dz.win, dgamma.win, M, Cc)
    torch.cuda.synchronize()
    s = R.row_scale(rowscale, rps, M)
    # dz: the kernel evaluates s * gamma * g left to right, (s * gamma) * g, two fp32 products that no compiler may reassociate or
    # contract (there is no addition).  The reference multiplies in the same order in fp32, so the comparison is exact.
    assert_bits(dz.win, ((s * gamma) * g).to(tdt), "dz")
    dz.assert_canaries()
    terms = s.double() * g.double() * z.double()
    assert_within(dgamma.win, dg0.double() + terms.sum(0), R.summation_bound(M, dg0.double().abs() + terms.abs().sum(0)), "dgamma")
    dgamma.assert_canaries()


def test_layerscale_bwd_refuses_more_than_1024_columns():
    """One lane per 4 columns, 256 lanes a workgroup: the limit is C = 1024, and the host names it."""
    M, Cc = 2, 1028
    g = torch.zeros(M, Cc, device="cuda")
    dz = torch.zeros(M, Cc, device="cuda")
    dgamma = torch.zeros(Cc, device="cuda")
    with pytest.raises(L.LnxError, match="1024"):
        ops.layerscale_bwd(g, g, dgamma, None, 0, dz, dgamma, M, Cc)
    torch.cuda.synchronize()
    assert float(dz.abs().sum()) == 0 and float(dgamma.abs().sum()) == 0


# rows * ldp / 4 vectors: 2 * 257 * 257 * 8 = 1 056 784 and 3 * 134 * 132 * 20 = 1 061 280, both > 4096 * 256
@BOTH
@pytest.mark.parametrize("B,Cin,H,W,ldp", [(2, 1, 1028, 1028, 32), (3, 4, 536, 528, 80)])
def test_im2col_stem_grid_cap_padding(B, Cin, H, W, ldp, dtype):
    assert B * (H // 4) * (W // 4) * (ldp // 4) > 4096 * 256 and ldp > Cin * 16
    gen = cgen(B + Cin + dtype)
    x = randn(gen, B, Cin, H, W)
    rows = B * (H // 4) * (W // 4)
    pat = Guarded(rows, ldp, DT[dtype], NAN, gr=2, gc=0)  # the kernel owns whole rows of ldp columns: canary rows only
    ops.im2col_stem(x, pat.win)
    torch.cuda.synchronize()
    want = torch.zeros(rows, ldp, device="cuda", dtype=DT[dtype])
    want[:, :Cin * 16] = torch.nn.functional.unfold(x, 4, stride=4).transpose(1, 2).reshape(rows, Cin * 16).to(DT[dtype])
    assert_bits(pat.win, want, "im2col_stem")
    pat.assert_canaries()


def test_agg2_fwd_bwd_every_workgroup_loops():
    """M * C = 263 153 > 256 * 1024: the backward's 256 workgroups each take a second trip and add atomically."""
    M, Cc = 517, 509
    n = M * Cc
    assert n > 256 * 1024
    gen = cgen(41)
    a, b, dout = randn(gen, M, Cc), randn(gen, M, Cc), randn(gen, M, Cc)
    w2 = torch.tensor([0.7, -0.3], device="cuda")
    bias1 = torch.tensor([0.2], device="cuda")
    out = flat(n, torch.float32, NAN, (M, Cc))
    ops.agg2_fwd(a, b, w2, bias1, out.win, M, Cc)
    torch.cuda.synchronize()
    ta, tb = w2[0].double() * a.double(), w2[1].double() * b.double()
    # three roundings (two products, two sums, of which a contraction removes up to two): data_movement_ref.blend_bound
    assert_within(out.win, ta + tb + bias1.double(), R.blend_bound(ta, tb, bias1.double()), "agg2_fwd")
    out.assert_canaries()
    da, db = flat(n, torch.float32, NAN, (M, Cc)), flat(n, torch.float32, NAN, (M, Cc))
    dw0, dbias0 = randn(gen, 2), randn(gen, 1)
    dw2, dbias1 = flat(2, torch.float32, dw0), flat(1, torch.float32, dbias0)
    ops.agg2_bwd(dout, a, b, w2, da.win, db.win, dw2.win, dbias1.win, M, Cc)
    torch.cuda.synchronize()
    assert_bits(da.win, w2[0] * dout, "da")  # one fp32 product each: exact
    assert_bits(db.win, w2[1] * dout, "db")
    d64 = dout.double()
    for k, other in enumerate((a, b)):
        t = d64 * other.double()
        assert_within(dw2.win[k], dw0[k].double() + t.sum(), R.summation_bound(n, dw0[k].double().abs() + t.abs().sum()), f"dw2[{k}]")
    assert_within(dbias1.win[0], dbias0[0].double() + d64.sum(), R.summation_bound(n, dbias0[0].double().abs() + d64.abs().sum()), "dbias1")
    for t in (da, db, dw2, dbias1):
        t.assert_canaries()


# B * 16 = 592: two workgroups plus 80 lanes
@BOTH
@pytest.mark.parametrize("width,off,dim", [(19, 0, 16), (19, 18, 1)])
def test_pack_meta_edges(width, off, dim, dtype):
    B = 37
    assert (B * 16) % 256 != 0 and off + dim <= width
    meta = randn(cgen(51 + dim), B, width)
    out = Guarded(B, 16, DT[dtype], NAN, gr=2, gc=0)
    ops.pack_meta(meta, off, dim, out.win)
    torch.cuda.synchronize()
    want = torch.zeros(B, 16, device="cuda", dtype=DT[dtype])
    want[:, :dim] = meta[:, off:off + dim].to(DT[dtype])
    assert_bits(out.win, want, "pack_meta")
    out.assert_canaries()


# K = 4: one lane; K = 1028: one whole trip of the 1024-column stride plus one lane
@pytest.mark.parametrize("with_bias", [True, False], ids=["s_t", "s_only"])
@pytest.mark.parametrize("K", [4, 1028])
def test_layerscale_apply_wgrad(K, with_bias):
    Cc = 5
    gen = cgen(61 + K + with_bias)
    s = Guarded(Cc, K, torch.float32, randn(gen, Cc, K), gc=8)    # lds = K + 16
    w = Guarded(Cc, K, torch.float32, randn(gen, Cc, K), gc=16)   # ldw = K + 32
    dw0 = randn(gen, Cc, K)
    dw = Guarded(Cc, K, torch.float32, dw0, gc=24)                # lddw = K + 48
    gamma, dg0 = randn(gen, Cc), randn(gen, Cc)
    dgamma = flat(Cc, torch.float32, dg0)
    t = b = db = db0 = None
    if with_bias:
        t, b, db0 = randn(gen, Cc), randn(gen, Cc), randn(gen, Cc)
        db = flat(Cc, torch.float32, db0)
    ops.layerscale_apply_wgrad(s.win, t, w.win, b, gamma, dw.win, db.win if db else None, dgamma.win)
    torch.cuda.synchronize()
    gs = gamma.double()[:, None] * s.win.double()
    assert_within(dw.win, dw0.double() + gs, R.fma_bound(dw0.double(), gs), "dw")  # one fma an element
    terms = w.win.double() * s.win.double()
    ref, mag = dg0.double() + terms.sum(1), dg0.double().abs() + terms.abs().sum(1)
    if with_bias:
        gt = gamma.double() * t.double()
        assert_within(db.win, db0.double() + gt, R.fma_bound(db0.double(), gt), "db")
        db.assert_canaries()
        ref, mag = ref + b.double() * t.double(), mag + (b.double() * t.double()).abs()
    assert_within(dgamma.win, ref, R.summation_bound(K + 1, mag), "dgamma")  # K products and b t onto the value already there
    for x in (s, w, dw, dgamma):
        x.assert_canaries()


# =====================================================================================================================================
# 4. lnx_mix_rows
# =====================================================================================================================================
def run_mix(x, perm, valid, out, mode, *, lam=0.0, hw=None, box=None):
    a = L.MixArgs()
    a.x, a.perm, a.valid, a.out = x.data_ptr(), perm.data_ptr(), valid.data_ptr() if valid is not None else None, out.data_ptr()
    a.B, a.row, a.lam, a.mode = x.shape[0], x[0].numel(), lam, mode
    if mode == 1:
        (a.H, a.W), (a.h0, a.h1, a.w0, a.w1) = hw, box
    L.check(L.lib().lnx_mix_rows(C.byref(a), _stream()), "lnx_mix_rows")


def test_mix_rows_box_every_column_pair():
    """The CutMix paste uses 4-wide vectors whose ends need not be multiples of 4: all 153 (w0, w1) with 0 <= w0 <= w1 <= W (the 17
    empty ones and the full width among them), each at the top edge, the bottom edge and an interior band.  Exact."""
    B, Cn, H, W = 3, 2, 6, 16
    x = randn(cgen(71), B, Cn, H, W)
    perm = torch.tensor([1, 0, 2], device="cuda")  # sample 2 is its own partner
    valid = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")  # sample 1 is not mixable
    pairs = [(w0, w1) for w0 in range(W + 1) for w1 in range(w0, W + 1)]
    assert len(pairs) == 153 and (0, W) in pairs and (5, 5) in pairs
    for h0, h1 in [(0, 2), (4, H), (2, 5)]:
        for w0, w1 in pairs:
            out = Guarded(B, Cn * H * W, torch.float32, NAN, gr=1, gc=0)
            run_mix(x, perm, valid, out.win, 1, hw=(H, W), box=(h0, h1, w0, w1))
            want = R.mix_box(x, perm.tolist(), valid.tolist(), h0, h1, w0, w1)
            assert_bits(out.win.view(B, Cn, H, W), want, f"box h {h0}:{h1} w {w0}:{w1}")
            out.assert_canaries()
            if w0 < w1:
                assert not torch.equal(want[0], x[0]) and torch.equal(want[1:], x[1:])  # exactly one sample really changes


@pytest.mark.parametrize("mode", [0, 2])
def test_mix_rows_blend(mode):
    """Row length 1500: a multiple of 4, not of 1024.  Mode 0 blends every sample, mode 2 only the valid ones (the others are
    copied, exactly).  lam a + (1 - lam) p: three roundings, data_movement_ref.blend_bound."""
    B, row = 3, 1500
    lam = float(torch.tensor(0.3, dtype=torch.float32))
    x = randn(cgen(72 + mode), B, row)
    perm = torch.tensor([1, 0, 2], device="cuda")
    valid = torch.tensor([1, 0, 1], dtype=torch.uint8, device="cuda")
    out = Guarded(B, row, torch.float32, NAN, gr=1, gc=0)
    run_mix(x, perm, valid if mode == 2 else None, out.win, mode, lam=lam)
    torch.cuda.synchronize()
    ref, bound = R.mix_blend(x, perm, lam)
    if mode == 2:
        assert_bits(out.win[1], x[1], "an invalid sample is copied")
        ref[1], bound[1] = x[1].double(), 0.0
    assert_within(out.win, ref, bound, f"mix_rows mode {mode}")
    out.assert_canaries()
