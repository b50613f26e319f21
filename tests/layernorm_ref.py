"""Plain float64 reference of lnx_layernorm_fwd / lnx_layernorm_bwd (include/lnx.h) on the CPU: what tests/test_gpu_layernorm.py
compares csrc/norm.hip against.

Operands are 2-D CPU tensors `[physical rows, leading dimension]` that already hold the values the kernel reads (rounded to the
storage type by the caller); columns beyond C are ignored, rows are picked with the row maps.  Results are compact `[M, C]`
float64 tensors in the order of the logical rows m = 0 .. M - 1; `rows(M, row_map)` says where row m lives in a mapped buffer."""
import torch


def rows(M, row_map=None):
    """Physical row of every logical row: m + (m / group) * pad + off, group == 0 = identity (lnx_rowmap)."""
    m = torch.arange(M, dtype=torch.int64)
    group, pad, off = row_map or (0, 0, 0)
    return m if group == 0 else m + (m // group) * pad + off


def forward(x, w, b, eps, M, C, *, x_map=None, add=None):
    """(y, mean, rstd) in float64: biased variance, eps inside the square root; `add` ([>= M, >= C], compact rows) is added to y."""
    xr = x[rows(M, x_map), :C].double()
    mean = xr.mean(-1)
    xc = xr - mean[:, None]
    rstd = 1.0 / torch.sqrt((xc * xc).mean(-1) + eps)
    y = xc * rstd[:, None] * w.double()[:C] + b.double()[:C]
    if add is not None:
        y = y + add[:M, :C].double()
    return y, mean, rstd


def stats_fp32(x, eps, M, C, *, x_map=None):
    """The fp32 mean / rstd arrays the backward takes as inputs: the float64 statistics rounded once."""
    _, mean, rstd = forward(x, torch.ones(C), torch.zeros(C), eps, M, C, x_map=x_map)
    return mean.float(), rstd.float()


def backward(dy, x, w, mean, rstd, M, C, *, dy_map=None, x_map=None, gin=None, relu_mask=False, dx2_rowscale=None, dx2_rows_per_sample=0):
    """dict of float64 tensors.  mean / rstd ([M] fp32) are inputs of the operation, used as given.
      dx  [M, C]  rstd (g - mean(g) - xhat mean(g xhat)) (+ gin, read through x_map) (x (x > 0) with relu_mask),  g = dy w
      dx2 [M, C]  dx2_rowscale[m / dx2_rows_per_sample] dx   (dx itself without a rowscale)
      dw, db [C]  sum_m dy xhat,  sum_m dy
      dw_abs, db_abs [C]  sum_m |dy xhat|,  sum_m |dy|: the magnitudes a column sum's rounding error is relative to"""
    xr = x[rows(M, x_map), :C].double()
    dyr = dy[rows(M, dy_map), :C].double()
    xhat = (xr - mean.double()[:, None]) * rstd.double()[:, None]
    g = dyr * w.double()[:C]
    dx = rstd.double()[:, None] * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    if gin is not None:
        dx = dx + gin[rows(M, x_map), :C].double()
    if relu_mask:
        dx = dx * (xr > 0).double()
    dx2 = dx
    if dx2_rowscale is not None:
        dx2 = dx * dx2_rowscale.double()[torch.arange(M) // dx2_rows_per_sample][:, None]
    t = dyr * xhat
    return {"dx": dx, "dx2": dx2, "dw": t.sum(0), "db": dyr.sum(0), "dw_abs": t.abs().sum(0), "db_abs": dyr.abs().sum(0)}
