"""Plain torch restatement of the small data-movement kernels (linnaeus_amd/csrc/elementwise.hip, the row mixing of collate.hip),
for tests/test_gpu_data_movement.py.  Everything runs on whatever device its inputs live on; arithmetic references are float64.

Copies and casts are exact (a cast to bf16 is round-to-nearest-even, which is what Tensor.to(torch.bfloat16) does), a single fp32
product is exact against the same product in torch, so those references are compared bit for bit.  The only error bounds are

  fma_bound        |a| + |b| scaled by 2^-23: one rounding of a product plus one of a sum (u = 2^-24 each, relative to a value no
                   larger than |a| + |b|), which holds whether or not the compiler contracts the pair into one fma
  blend_bound      w0 a + w1 b (+ c): three roundings, each relative to a partial result no larger than |w0 a| + |w1 b| + |c|, so
                   3u <= 2 * 2^-23 of that sum, contracted or not
  summation_bound  the worst-case bound of an fp32 sum of n terms in any order, (n - 1) u sum|terms|, plus 2 u sum|terms| for the
                   (at most two) roundings inside each term, plus one u of slack for the second-order terms: (n + 2) u sum|terms|
"""
import torch

U = 2.0 ** -24  # unit roundoff of fp32


def bits(t):
    """The storage bits of a float32 / bfloat16 tensor as integers (so that -0.0 != 0.0 and NaN == NaN)."""
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def map_rows(M, row_map, device):
    """Row index of every m in [0, M) under the (group, pad, off) row map: m + (m // group) * pad + off."""
    m = torch.arange(M, device=device)
    group, pad, off = row_map
    return m + (m // group) * pad + off if group > 0 else m


def row_scale(rowscale, rows_per_sample, M):
    """rowscale[m // rows_per_sample] for every m in [0, M), as a column."""
    return rowscale[torch.arange(M, device=rowscale.device) // rows_per_sample][:, None]


def fma_bound(a, b):
    return 2.0 ** -23 * (a.abs() + b.abs())


def blend_bound(*terms):
    return 2.0 * 2.0 ** -23 * sum(t.abs() for t in terms)


def summation_bound(n, abs_sum):
    return (n + 2) * U * abs_sum


# --- lnx_prep_weights ---------------------------------------------------------------------------------------------------------------
def prep_logical(src, conv_perm_p=0):
    """The operand as the GEMMs see it, [rows, cols] fp32: the source itself, or for the 2x2-conv layout its columns regrouped from
    (channel, position) to (position, channel)."""
    if not conv_perm_p:
        return src
    n, k = src.shape
    return src.view(n, k // conv_perm_p, conv_perm_p).permute(0, 2, 1).reshape(n, k)


def prep_main(src, ld, dtype, conv_perm_p=0):
    """[rows, ld] of dtype: the cast operand with columns cols..ld-1 zero."""
    rows, cols = src.shape
    out = torch.zeros(rows, ld, dtype=dtype, device=src.device)
    out[:, :cols] = prep_logical(src, conv_perm_p).to(dtype)
    return out


def prep_transposed(src, dtype, conv_perm_p=0):
    """[cols, rows] of dtype: the block of the transposed copy that the kernel writes (columns rows..ld_t-1 are the caller's)."""
    return prep_logical(src, conv_perm_p).to(dtype).t().contiguous()


def prep_dw49(src):
    """[C, 49] -> tap-major fp32 [49, C]."""
    return src.t().contiguous()


# --- dropout ------------------------------------------------------------------------------------------------------------------------
def dropout_mul(x, mask, inv_keep):
    """where(mask != 0, x * inv_keep, 0) in fp32, rounded to the type of x.  inv_keep: a Python float that is an fp32 value."""
    y = torch.where(mask != 0, x.float() * inv_keep, torch.zeros((), device=x.device))
    return y.to(x.dtype)


def dropout_residual(z, mask, inv_keep, rowscale, rows_per_sample, res):
    """(float64 reference, bound) of res + z * fp32(rowscale * inv_keep) where the mask keeps; where it drops the reference is res
    and the bound is zero."""
    M = z.shape[0]
    ik = torch.tensor(inv_keep, dtype=torch.float32, device=z.device)
    rs32 = row_scale(rowscale, rows_per_sample, M) * ik if rowscale is not None else (torch.ones((), device=z.device) * ik).reshape(1, 1)
    term = z.double() * rs32.double()
    keep = mask != 0
    ref = torch.where(keep, res.double() + term, res.double())
    bound = torch.where(keep, fma_bound(res.double(), term), torch.zeros((), dtype=torch.float64, device=z.device))
    return ref, bound


# --- lnx_mix_rows -------------------------------------------------------------------------------------------------------------------
def mix_box(x, perm, valid, h0, h1, w0, w1):
    """x [B, C, H, W]: the box [h0, h1) x [w0, w1) of every valid sample replaced by its partner's."""
    out = x.clone()
    for b in range(x.shape[0]):
        if valid[b]:
            out[b, :, h0:h1, w0:w1] = x[int(perm[b]), :, h0:h1, w0:w1]
    return out


def mix_blend(x, perm, lam):
    """(float64 reference, bound) of lam x[b] + fp32(1 - lam) x[perm[b]].  lam: a Python float that is an fp32 value."""
    m = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(lam, dtype=torch.float32))
    a, p = x.double() * lam, x[perm].double() * m
    return a + p, blend_bound(a, p)
