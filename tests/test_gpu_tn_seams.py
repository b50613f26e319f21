"""The weight-gradient GEMMs (lnx_gemm_tn: gemm_tn_kernel<T> of gemm.hip, the four gemm_tn_v2_kernel<RW, CW, PATCH> instantiations of
gemm2.hip, the second stages gemm_tn_reduce_kernel / gemm_tn_reduce_batch_kernel) at every ring length, split seam and tile form,
against the exact reference of tests/tn_ref.py.

Method, for every case: lnx_gemm_tn_query first, and the case asserts the kernel, tile form, patch flag, split and summation path it
was written for; operands are integers in {-3 .. 3} inside NaN storage, dW / db start at 5.0 inside sentinel guards; after the call the
guards are untouched, no NaN has reached the stored part and EVERY element equals the fp64 reference bit for bit (fp32 sums of these
integers are exact in any order -- tn_ref's docstring; tests/test_tn_ref_host.py checks the bound for every case).  A workspace is
sized exactly for the launch and pre-filled with NaN: where the workspace path is expected its first tile is finite afterwards, where
atomics are expected it is still all NaN; eight NaN floats behind it must stay NaN either way."""
import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests import tn_ref as T

pytestmark = pytest.mark.gpu
DT = {"bf16": L.BF16, "f32": L.F32}
WS_TAIL = 8

_inputs = {}


def inputs_of(c: T.Case):
    """dY / A of a case on the device, built once for all cases that read the same operands (they are never written)"""
    key = (c.dtype, c.M, c.N, c.K, c.lddy, c.patch, c.m_eff)
    if key not in _inputs:
        if len(_inputs) >= 6:
            _inputs.pop(next(iter(_inputs)))
        _inputs[key] = T.Inputs(c, "cuda")
    return _inputs[key]


class Run:
    """one lnx_gemm_tn call of a case: query, assert the path, launch, and what is needed to check it afterwards"""

    def __init__(self, c: T.Case, ws_floats=None, defer=False, check_path=True):
        self.c, self.inp, self.out = c, inputs_of(c), T.Outputs(c, "cuda")
        inp, out = self.inp, self.out
        q_host, ws_floats = T.query_case(c, ws_floats)
        self.ws_store = torch.full((ws_floats + WS_TAIL,), T.NAN, device="cuda") if c.ws else None
        self.ws = self.ws_store[:ws_floats] if c.ws else None
        self.m_dev = torch.tensor([c.m_eff], dtype=torch.int32, device="cuda") if c.m_eff is not None else None
        kw = dict(M=c.M, N=c.N, K=c.K, lda=inp.lda, lddw=out.lddw, db=out.db, a_patch=inp.a_patch, k_perm_c=c.k_perm_c, k_store=c.k_store, splits=c.hint,
                  dtype=DT[c.dtype], ws=self.ws, m_dev=self.m_dev, defer=defer)
        assert inp.dY.stride(0) == inp.lddy and out.dW.stride(0) == out.lddw
        self.q = q = ops.gemm_tn_query(inp.dY, inp.A, out.dW, **kw)
        # the query of the real arguments is the query of the sizes alone
        fields = [f for f, _ in L.TnLaunch._fields_]
        assert [getattr(q, f) for f in fields] == [getattr(q_host, f) for f in fields]
        if check_path:
            T.assert_path(c, q)
        ops.gemm_tn(inp.dY, inp.A, out.dW, **kw)

    def check_workspace(self):
        if self.ws_store is None:
            return
        c, q = self.c, self.q
        assert bool(torch.isnan(self.ws_store[-WS_TAIL:]).all()), f"{c.id}: the kernel wrote behind its workspace"
        if not q.workspace:
            assert bool(torch.isnan(self.ws_store).all()), f"{c.id}: atomics were expected, but the workspace was written"
            return
        tile = q.rw * q.cw
        tiles = q.tiles_n * q.tiles_k
        assert bool(torch.isfinite(self.ws[:tile]).all()), f"{c.id}: the first partial tile is not finite"
        assert T.ws_need(q) == self.ws.numel()
        if c.N % 8 == 0:
            # (with N % 8 != 0 the clamped chunk carries dY's NaN padding into rows n >= N of the last row of tiles, which are stored
            # unmasked and masked by the second stage: legal there, and the exact comparison of dW shows that they stay there)
            assert bool(torch.isfinite(self.ws[:q.splits * tiles * tile]).all()), f"{c.id}: a partial tile was not stored (or holds NaN)"
        if c.m_eff is not None:
            # every split takes its range from the effective count: ceil(tiles of 64 / splits) tiles each; a split left without rows
            # stores zeros (the second stage sums every slot)
            m = max(0, min(c.M, c.m_eff))
            per = T.cdiv(T.cdiv(m, 64), q.splits) * 64
            for s in range(q.splits):
                if s * per >= m:
                    part = self.ws[s * tiles * tile:(s + 1) * tiles * tile]
                    assert bool((part == 0).all()), f"{c.id}: surplus split {s} left something other than zeros in the workspace"

    def check(self):
        torch.cuda.synchronize()
        self.out.check(self.inp)
        self.check_workspace()


def ids(cases):
    return [c.id for c in cases]


@pytest.mark.parametrize("c", T.RING_SPLIT_CASES, ids=ids(T.RING_SPLIT_CASES))
def test_ring_length_and_split_seams(c):
    """gemm_tn_v2_kernel<256,128,false> / <128,256,false> on one full tile with 1, 2, 3, 4, 5, 7, 10, 64 and 8 contraction tiles per split
    (the prologue / drain cases of the 3-stage ring), a ragged last split, and the second stage with 64, 32, 22, 16, 13, 10, 7 splits
    (batches of 8, remainder, both); with and without workspace, with and without db."""
    Run(c).check()


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("form", [T.WIDE_R, T.WIDE_C], ids=["256x128", "128x256"])
def test_workspace_smaller_than_the_launch_needs(form, deterministic):
    """hint 16 with a workspace that holds 8 splits: default mode keeps the 16 splits and falls back to atomics (workspace untouched),
    deterministic mode splits less -- 9 would fit, which is 8 tiles per split, 8 splits -- and sums in the workspace."""
    n, k = T.ONE_TILE[form]
    have = 8 * 256 * 128 + 8 * form[0]
    c = T.ring_case(n, k, form, 16, splits=8 if deterministic else 16, m_per_split=512 if deterministic else 256, workspace=deterministic)
    prev = L.set_deterministic(deterministic)
    try:
        r = Run(c, ws_floats=have)
        r.check()
    finally:
        L.set_deterministic(prev)
    assert L.is_deterministic() == prev


@pytest.mark.parametrize("c", T.RING_EDGE_CASES, ids=ids(T.RING_EDGE_CASES))
def test_ring_tile_edges_k_store_and_permutation(c):
    """Several tiles with ragged edges in both forms, N % 8 != 0 (the loader's clamped chunk reads dY's NaN padding), sparse tiles that
    stay on the atomics, k_store / lddw (the stem's form; the mask of the atomics epilogue and of the second stage) and k_perm_c."""
    Run(c).check()


@pytest.mark.parametrize("c", T.RING_PATCH_CASES, ids=ids(T.RING_PATCH_CASES))
def test_ring_patch_gather(c):
    """gemm_tn_v2_kernel<256,128,true> and <128,256,true> (the model's 192 -> 384 downsample among them): the incremental patch
    addressing (pr / po / qa / qb and the wrap carry) at Wo = 7, 14, 28, 12, 5, 64, 96 and 1, from m_begin = 0 and from an m_begin inside
    an image row; with m_dev a ragged last tile that ends inside an image row."""
    Run(c).check()


@pytest.mark.parametrize("c", T.M_DEV_CASES, ids=ids(T.M_DEV_CASES))
def test_m_dev_at_contraction_tile_seams(c):
    """m_eff in {0, 1, 63, 64, 65, M - 1, M, M + 7} on both kernels' single-tile shapes: rows at and behind m_eff hold NaN, surplus splits
    leave zeros in the workspace and nothing in dW."""
    Run(c).check()


@pytest.mark.parametrize("c", T.V1_CASES, ids=ids(T.V1_CASES))
def test_128x128_kernel(c):
    """gemm_tn_kernel<bf16> / <float>: M below, at and one past a contraction tile, a hint larger than the ranges it can fill, N and K one
    chunk past a tile, the meta head's k_store = lddw form, fp32 with the patch gather, m_dev, and bf16 at M % 64 != 0 above 4096."""
    Run(c).check()


def test_deferred_second_stages():
    """Three products (one per tile form, one with the patch gather), each with its own workspace, deferred and summed by ONE
    lnx_gemm_tn_flush: nothing reaches dW / db before the flush; afterwards they equal the exact reference -- and therefore the same
    three run undeferred, which are checked the same way."""
    L.lib().lnx_gemm_tn_discard()
    now = [Run(c) for c in T.DEFER_CASES]
    for r in now:
        r.check()
    later = [Run(c, defer=True) for c in T.DEFER_CASES]
    torch.cuda.synchronize()
    try:
        for r in later:
            assert r.q.workspace == 1
            assert bool((r.out.dW == T.INIT).all()) and bool((r.out.db == T.INIT).all()), f"{r.c.id}: summed before the flush"
        ops.gemm_tn_flush()
    finally:
        L.lib().lnx_gemm_tn_discard()
    for r, r0 in zip(later, now):
        r.check()
        assert torch.equal(r.out.dW_store, r0.out.dW_store) and torch.equal(r.out.db_store, r0.out.db_store)
