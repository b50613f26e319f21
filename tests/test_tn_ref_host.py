"""tests/tn_ref.py checked on the host: the exact reference of the weight-gradient seam tests against torch's own conv2d weight gradient,
the comparator shown to bite, and the arithmetic that makes "bit for bit" a fair demand of every case in the tables.  No GPU."""
import pytest
import torch

from tests import tn_ref as T


def conv_weight_grad(x, dY, N):
    """weight gradient [N, Cin, 2, 2] of a 2x2 / stride-2 conv over x [B, Hin, Win, Cin] (NHWC) for output gradient rows dY [B Ho Wo, N]"""
    B, Hin, Win, Cin = x.shape
    w = torch.zeros(N, Cin, 2, 2, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), w, stride=2)
    y.backward(dY.double().view(B, Hin // 2, Win // 2, N).permute(0, 3, 1, 2))
    return w.grad


@pytest.mark.parametrize("B,Ho,Wo,Cin,N", [(2, 3, 5, 4, 6), (1, 1, 1, 8, 3), (3, 2, 7, 8, 5), (2, 13, 5, 12, 4)])
def test_patch_gather_and_column_permutation_against_conv2d(B, Ho, Wo, Cin, N):
    gen = torch.Generator().manual_seed(B + Ho + Wo)
    x = T.draw(gen, B, 2 * Ho, 2 * Wo, Cin)
    dY = T.draw(gen, B * Ho * Wo, N)
    ref, ref_b = T.product(dY, T.patch_rows(x), B * Ho * Wo)
    g = conv_weight_grad(x, dY, N)
    # plain column order k = (kh * 2 + kw) * Cin + c  <->  [N, kh, kw, c]
    assert torch.equal(T.expected_dw(ref, 4 * Cin, init=0.0), g.permute(0, 2, 3, 1).reshape(N, 4 * Cin))
    # k_perm_c = Cin: the conv weight layout [N, Cin, kh, kw] as it lies in memory
    assert torch.equal(T.expected_dw(ref, 4 * Cin, k_perm_c=Cin, init=0.0), g.reshape(N, 4 * Cin))
    assert torch.equal(ref_b, dY.double().sum(0))
    # the initial value is added, not replaced
    assert torch.equal(T.expected_dw(ref, 4 * Cin, k_perm_c=Cin), g.reshape(N, 4 * Cin) + T.INIT)


def test_patch_row_of_source_is_the_inverse_of_the_gather():
    B, Ho, Wo, Cin = 2, 3, 5, 4
    rows = T.patch_row_of_source(B, Ho, Wo)
    x = rows.to(torch.float32).unsqueeze(-1).expand(B, 2 * Ho, 2 * Wo, Cin).contiguous()
    A = T.patch_rows(x)
    assert torch.equal(A, torch.arange(B * Ho * Wo, dtype=torch.float32).unsqueeze(1).expand(-1, 4 * Cin))


def test_k_store_cut_and_permutation_columns():
    ref = torch.arange(3 * 16, dtype=torch.float64).view(3, 16) + 1
    out = T.expected_dw(ref, 11, k_store=11, init=0.0)
    assert torch.equal(out, ref[:, :11])
    col = T.stored_column(16, 4)
    assert sorted(col.tolist()) == list(range(16)) and col[5].item() == 1 * 4 + 1 and col[4].item() == 1  # k = p C + c -> c P + p
    cut = T.expected_dw(ref, 16, k_perm_c=4, k_store=13, init=0.0)
    assert int((cut != 0).sum()) == 3 * 13 and torch.equal(cut[:, col[:13]], ref[:, :13])
    assert torch.equal(T.expected_dw(ref, 16, k_store=16, init=0.0), ref) and torch.equal(T.expected_dw(ref, 16, k_store=99, init=0.0), ref)


SMALL = [T.Case("f32", 70, 9, 8, kernel=T.V1), T.Case("bf16", 70, 9, 16, k_store=11, lddw=11, kernel=T.V1),
         T.Case("f32", 30, 6, 16, patch=(2, 3, 5, 4), k_perm_c=4, k_store=13, kernel=T.V1), T.Case("bf16", 70, 9, 8, m_eff=33, kernel=T.V1, db=False)]


@pytest.mark.parametrize("c", SMALL, ids=[c.id for c in SMALL])
def test_the_comparator_bites(c):
    """Outputs.check passes on the reference itself and fails on: a contraction row dropped, a row doubled, a touched guard, a NaN."""
    inp, out = T.Inputs(c, "cpu"), T.Outputs(c, "cpu")
    want_w, want_b = out.expected(inp)
    clean_w, clean_b = want_w.clone(), want_b.clone()

    def put(w, b):
        out.dW_store.copy_(w)
        out.db_store.copy_(b)

    put(clean_w, clean_b)
    out.check(inp)
    # the operands are what the kernel may read: NaN at and behind m_eff and around the windows, finite integers inside
    m = inp.m_eff
    assert torch.isnan(inp.dY_store[m:]).all() and torch.isnan(inp.dY_store[:, c.N:]).all() and not torch.isnan(inp.dY_store[:m, :c.N]).any()
    assert inp.dY_store.shape[1] > c.N and out.dW_store.shape[0] > c.N
    # one contraction row removed from / added twice to the product
    a = T.patch_rows(torch.nan_to_num(inp.A.float())) if c.patch else torch.nan_to_num(inp.A.float())
    row = 17
    delta = torch.outer(inp.dY[row].double(), a[row].double())
    assert int((delta != 0).sum()) > 0
    for sign in (-1.0, 1.0):
        w = clean_w.clone()
        w[:c.N, :out.width] = T.expected_dw(inp.ref + sign * delta, out.width, c.k_perm_c, c.k_store).float()
        put(w, clean_b)
        with pytest.raises(AssertionError, match="dW differs"):
            out.check(inp)
    if c.db:
        b = clean_b.clone()
        b[:c.N] -= inp.dY[row].float()
        put(clean_w, b)
        with pytest.raises(AssertionError, match="db differs"):
            out.check(inp)
    # a guard row of dW, a guard entry of db, a NaN in the stored part
    w = clean_w.clone()
    w[c.N, 0] = 0.0
    put(w, clean_b)
    with pytest.raises(AssertionError, match="guard"):
        out.check(inp)
    b = clean_b.clone()
    b[c.N] = T.INIT
    put(clean_w, b)
    with pytest.raises(AssertionError, match="guard"):
        out.check(inp)
    w = clean_w.clone()
    w[0, 0] = T.NAN
    put(w, clean_b)
    with pytest.raises(AssertionError, match="NaN"):
        out.check(inp)
    put(clean_w, clean_b)
    out.check(inp)


def test_m_eff_rows_of_a_patch_source_are_poisoned_exactly():
    c = T.Case("f32", 30, 6, 16, patch=(2, 3, 5, 4), k_perm_c=4, m_eff=7, kernel=T.V1)
    inp = T.Inputs(c, "cpu")
    A = T.patch_rows(inp.A.float())
    assert torch.isnan(A[7:]).all() and not torch.isnan(A[:7]).any()
    assert torch.isnan(inp.A_store[inp.A.numel():]).all()


def all_cases():
    return [(name, c) for name, cases in T.ALL_TABLES.items() for c in cases]


def test_every_case_keeps_fp32_sums_exact():
    """9 M + |init| < 2**24 for every case of every table: each product is an integer of magnitude <= 9, so every partial sum in any order
    is an integer below 2**24 and fp32 holds it exactly; the operands themselves ({-3 .. 3}) are exact in bf16."""
    assert len(all_cases()) > 300
    for name, c in all_cases():
        assert T.max_abs_sum(c.M) < 2**24 and c.M <= 8192, (name, c.id)
    for v in range(-3, 4):
        assert torch.tensor(float(v)).bfloat16().float().item() == v
    gen = torch.Generator().manual_seed(0)
    d = T.draw(gen, 7000)
    assert sorted(d.unique().tolist()) == [-3, -2, -1, 0, 1, 2, 3] and all(abs(int((d == v).sum()) - 1000) < 150 for v in range(-3, 4))


def test_case_tables_are_well_formed():
    """ids are unique within a table; ring cases are bf16 with M % 64 == 0 and M >= 4096, the others are not; the split hints of the
    ring table give the tiles per split the table's comment promises; every operand stays below 10 MB."""
    for name, cases in T.ALL_TABLES.items():
        assert len({c.id for c in cases}) == len(cases), name
    for name, c in all_cases():
        ring_ok = c.dtype == "bf16" and c.M % 64 == 0 and c.M >= 4096
        assert ring_ok == (c.kernel == T.RING), (name, c.id)
        esz = 2 if c.dtype == "bf16" else 4
        assert (c.M + T.EXTRA_ROWS) * max(T.lddy_of(c), c.K + 8) * esz < 10e6, (name, c.id)
        if c.patch:
            B, Ho, Wo, Cin = c.patch
            assert c.M == B * Ho * Wo and c.K == 4 * Cin and c.k_perm_c == Cin, (name, c.id)
    per = {}
    for c in T.RING_SPLIT_CASES:
        if c.M == 4096 and c.hint > 0:
            per[c.hint] = (c.m_per_split // 64, 64 - (c.splits - 1) * (c.m_per_split // 64))
    assert per == {64: (1, 1), 32: (2, 2), 22: (3, 1), 16: (4, 4), 13: (5, 4), 10: (7, 1), 7: (10, 4), 1: (64, 64)}
    # the hinted patch cases start a split inside an image row wherever a multiple of 64 can
    hinted = [c for c in T.RING_PATCH_CASES if c.hint > 0 and c.m_eff is None]
    assert len(hinted) == len(T.PATCH_FORMS) * len(T.PATCH_GEOMS)
    for c in hinted:
        Wo = c.patch[2]
        assert c.m_per_split % Wo != 0 or Wo in (1, 64), c.id
