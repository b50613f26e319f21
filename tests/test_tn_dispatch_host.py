"""lnx_gemm_tn_query on the host: the launch decision of the weight-gradient GEMM (gemm_tn_dispatch.cpp: tn_plan, the function
lnx_gemm_tn itself launches from) pinned for the model's own products, DESIGN.md's TN table checked against it, and every case of the
seam tests' tables (tests/tn_ref.py) shown to be written for the path it names.  No GPU.

    python tests/test_tn_dispatch_host.py        prints the table of DESIGN.md section 6a"""
import ctypes as C
import os
import re

import pytest

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from tests import tn_ref as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 256  # images per GPU of the benchmark

# mFormerV1_sm at 224 x 224, 256 images, bf16 (the meta heads run in fp32); every product gets the plan's workspace of LNX_TN_WS_FLOATS.
# (name, dtype, M, N, K, k_store, patch source (Hin, Win, Cin) or None) -> (kernel, rw, cw, patch, splits, m_per_split, workspace)
MODEL_PRODUCTS = [
    (("stem", "bf16", B * 3136, 96, 64, 48, None), ("ring", 256, 128, 0, 256, 3136, 0)),
    (("conv-MLP C=96 fc1", "bf16", B * 3136, 384, 96, 0, None), ("ring", 256, 128, 0, 128, 6272, 0)),
    (("conv-MLP C=96 fc2", "bf16", B * 3136, 96, 384, 0, None), ("ring", 128, 256, 0, 128, 6272, 0)),
    (("downsample 96->192", "bf16", B * 784, 192, 384, 0, (56, 56, 96)), ("ring", 256, 128, 1, 85, 2368, 1)),
    (("conv-MLP C=192 fc1", "bf16", B * 784, 768, 192, 0, None), ("ring", 256, 128, 0, 42, 4800, 1)),
    (("conv-MLP C=192 fc2", "bf16", B * 784, 192, 768, 0, None), ("ring", 256, 128, 0, 42, 4800, 1)),
    (("downsample 192->384", "bf16", B * 196, 384, 768, 0, (28, 28, 192)), ("ring", 128, 256, 1, 28, 1792, 1)),
    (("RoPE C=384 qkv", "bf16", B * 199, 1152, 384, 0, None), ("ring", 256, 128, 0, 17, 3008, 1)),
    (("RoPE C=384 proj", "bf16", B * 199, 384, 384, 0, None), ("ring", 256, 128, 0, 42, 1216, 1)),
    (("RoPE C=384 fc1", "bf16", B * 199, 1536, 384, 0, None), ("ring", 256, 128, 0, 14, 3648, 1)),
    (("RoPE C=384 fc2", "bf16", B * 199, 384, 1536, 0, None), ("ring", 128, 256, 0, 14, 3648, 1)),
    (("downsample 384->768", "bf16", B * 49, 768, 1536, 0, (14, 14, 384)), ("ring", 256, 128, 1, 7, 1792, 1)),
    (("RoPE C=768 qkv", "bf16", B * 52, 2304, 768, 0, None), ("ring", 256, 128, 0, 4, 3328, 1)),
    (("RoPE C=768 proj", "bf16", B * 52, 768, 768, 0, None), ("ring", 256, 128, 0, 14, 960, 1)),
    (("RoPE C=768 fc1", "bf16", B * 52, 3072, 768, 0, None), ("ring", 256, 128, 0, 3, 4480, 1)),
    (("RoPE C=768 fc2", "bf16", B * 52, 768, 3072, 0, None), ("ring", 256, 128, 0, 3, 4480, 1)),
    (("head (1000 classes)", "bf16", B, 1000, 768, 0, None), ("128x128", 128, 128, 0, 1, 256, 0)),
    (("meta head hidden", "f32", B, 384, 384, 0, None), ("128x128", 128, 128, 0, 2, 128, 0)),
    (("meta head input (dim 4)", "f32", B, 384, 16, 4, None), ("128x128", 128, 128, 0, 2, 128, 0)),
]
KERNEL_NAME = {L.TN_KERNEL_V1: "128x128", L.TN_KERNEL_RING: "ring"}
BEGIN, END = "<!-- tn-dispatch-table-begin -->", "<!-- tn-dispatch-table-end -->"


def query(name, dtype, M, N, K, k_store, patch):
    q = ops.gemm_tn_query_shape(dtype=L.BF16 if dtype == "bf16" else L.F32, M=M, N=N, K=K, k_store=k_store, a_patch=patch, k_perm_c=patch[2] if patch else 0,
                                ws_floats=L.TN_WS_FLOATS)
    return (KERNEL_NAME[q.kernel], q.rw, q.cw, q.patch, q.splits, q.m_per_split, q.workspace)


def table():
    rows = ["| product | type | M | N | K | k_store | kernel | tile (N x K) | patch | splits | rows per split | partial tiles |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for (name, dtype, M, N, K, ks, patch), _ in MODEL_PRODUCTS:
        k, rw, cw, pt, sp, mps, ws = query(name, dtype, M, N, K, ks, patch)
        rows.append(f"| {name} | {dtype} | {M} | {N} | {K} | {ks or '-'} | {k} | {rw}x{cw} | {'yes' if pt else 'no'} | {sp} | {mps} | {'workspace' if ws else 'atomics'} |")
    return "\n".join(rows)


@pytest.mark.parametrize("product,expected", MODEL_PRODUCTS, ids=[p[0][0].replace(" ", "_") for p in MODEL_PRODUCTS])
def test_model_products_launch_as_recorded(product, expected):
    """The launch of every weight-gradient product of mFormerV1_sm at the benchmark's batch, recorded when the decision moved into
    tn_plan (it was held against a transcription of the rule as it stood in lnx_gemm_tn / launch_tn_v2 on 40 000 random argument sets, both
    modes): a change of the dispatch rule shows up here (and in DESIGN.md) before it shows up in a profile."""
    assert query(*product) == expected


def test_design_tn_table_is_what_the_library_decides():
    with open(os.path.join(REPO, "DESIGN.md")) as fh:
        doc = fh.read()
    m = re.search(re.escape(BEGIN) + r"\n(.*?)\n" + re.escape(END), doc, flags=re.S)
    assert m is not None, "DESIGN.md has no TN dispatch-table markers"
    assert m.group(1).strip() == table().strip(), "DESIGN.md's TN table is stale: python tests/test_tn_dispatch_host.py prints the current one"


def test_the_rules_the_seam_tests_rely_on():
    def q(**kw):
        kw.setdefault("dtype", L.BF16)
        return ops.gemm_tn_query_shape(**kw)

    # the ring kernel needs bf16, M % 64 == 0, M >= 4096
    assert q(M=4096, N=256, K=128).kernel == L.TN_KERNEL_RING and q(M=4096 + 32, N=256, K=128).kernel == L.TN_KERNEL_V1
    assert q(M=4032, N=256, K=128).kernel == L.TN_KERNEL_V1 and q(M=4096, N=256, K=128, dtype=L.F32).kernel == L.TN_KERNEL_V1
    # orientation by padding waste, ties to 256x128
    assert (q(M=4096, N=256, K=128).rw, q(M=4096, N=128, K=256).rw, q(M=4096, N=384, K=384).rw, q(M=4096, N=200, K=192).rw) == (256, 128, 256, 256)
    # automatic split: at least 8 contraction tiles each, at most one round of 256 workgroups; a hint is capped at one tile per split
    assert (q(M=4096, N=256, K=128).splits, q(M=64 * 4096, N=256, K=128).splits, q(M=64 * 4096, N=512, K=512).splits) == (8, 256, 32)
    assert q(M=4096, N=256, K=128, splits=1000).splits == 64 and q(M=4096, N=256, K=128, splits=1000).m_per_split == 64
    # a ragged last split: 64 tiles in splits of 3 -> 22 launched, not the 24 asked for
    r = q(M=4096, N=256, K=128, splits=24)
    assert (r.splits, r.m_per_split) == (22, 192)
    # workspace: only with one that is large enough, two or more splits and well-filled tiles
    need = 8 * 256 * 128 + 8 * 256
    assert q(M=4096, N=256, K=128, ws_floats=need).workspace == 1 and q(M=4096, N=256, K=128, ws_floats=need - 1).workspace == 0
    assert q(M=4096, N=256, K=128).workspace == 0 and q(M=4096, N=256, K=128, splits=1, ws_floats=need).workspace == 0
    assert q(M=4096, N=264, K=136, ws_floats=L.TN_WS_FLOATS).workspace == 0 and q(M=4096, N=256, K=128, k_store=80, ws_floats=need).workspace == 0
    # the patch flag follows a_mode on both kernels
    assert q(M=4096, N=256, K=128, a_patch=(128, 128, 32)).patch == 1 and q(M=64, N=256, K=128, a_patch=(16, 16, 32)).patch == 1


def test_query_refuses_what_the_launch_refuses():
    lib = L.lib()
    out = L.TnLaunch()
    a = L.WgradArgs()
    a.dtype = 7
    assert lib.lnx_gemm_tn_query(C.byref(a), C.byref(out)) != 0 and b"dtype" in lib.lnx_last_error()
    a.dtype, a.M, a.N, a.K, a.lddy, a.lda = L.BF16, 64, 8, 12, 8, 16
    assert lib.lnx_gemm_tn_query(C.byref(a), C.byref(out)) != 0 and b"multiple" in lib.lnx_last_error()
    assert lib.lnx_gemm_tn(C.byref(a), None) != 0 and b"multiple" in lib.lnx_last_error()
    a.K, a.lddy = 16, 4
    assert lib.lnx_gemm_tn_query(C.byref(a), C.byref(out)) != 0 and b"lddy" in lib.lnx_last_error()
    a.lddy = 8
    assert lib.lnx_gemm_tn_query(C.byref(a), None) != 0
    assert lib.lnx_gemm_tn_query(C.byref(a), C.byref(out)) == 0 and out.kernel == L.TN_KERNEL_V1  # no operand pointer is needed
    assert lib.lnx_gemm_tn(C.byref(a), None) != 0 and b"null operand" in lib.lnx_last_error()
    assert lib.lnx_version() >= 114


def test_deterministic_mode_in_the_query():
    """Deterministic mode: the 128x128 kernel is not split; the ring kernel's splits always meet in the workspace, and are made fewer until it
    holds them (none: one workgroup per tile)."""
    kw = dict(dtype=L.BF16, M=4096, N=256, K=128)
    need8 = 8 * 256 * 128 + 8 * 256
    prev = L.set_deterministic(True)
    try:
        q = ops.gemm_tn_query_shape(splits=16, ws_floats=need8, **kw)
        assert (q.splits, q.m_per_split, q.workspace) == (8, 512, 1)
        q = ops.gemm_tn_query_shape(splits=16, **kw)
        assert (q.splits, q.m_per_split, q.workspace) == (1, 4096, 0)
        q = ops.gemm_tn_query_shape(dtype=L.F32, M=4096, N=128, K=128, splits=16)
        assert (q.kernel, q.splits) == (L.TN_KERNEL_V1, 1)
    finally:
        L.set_deterministic(prev)
    q = ops.gemm_tn_query_shape(splits=16, ws_floats=need8, **kw)
    assert (q.splits, q.m_per_split, q.workspace) == (16, 256, 0)


ALL_CASES = [(name, c) for name, cases in T.ALL_TABLES.items() for c in cases]


def test_every_seam_case_is_written_for_the_path_it_names():
    """Each case of tests/tn_ref.py states kernel, tile form, patch flag, summation path and (mostly) splits and rows per split; the GPU
    tests assert them before they run, and here the whole table is held against the query without a GPU."""
    for name, c in ALL_CASES:
        q, ws_floats = T.query_case(c)
        T.assert_path(c, q)
        assert ws_floats * 4 < 14e6, (name, c.id)
    covered = {(q.rw, q.cw, q.patch) for q in (T.query_case(c)[0] for _, c in ALL_CASES) if q.kernel == L.TN_KERNEL_RING}
    assert covered == {(256, 128, 0), (128, 256, 0), (256, 128, 1), (128, 256, 1)}


if __name__ == "__main__":
    print(BEGIN + "\n" + table() + "\n" + END)
