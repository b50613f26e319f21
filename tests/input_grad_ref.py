"""fp64 CPU references of the input-gradient kernels (include/lnx.h: lnx_stem_dgrad / lnx_col2im_stem / lnx_meta_input_grad) and the
exact probe data of their tests.  Restated from the definitions, not from the kernels: the stem's is torch's own transposed convolution."""
import torch
import torch.nn.functional as F


def stem_dgrad_ref(dy: torch.Tensor, w: torch.Tensor, B: int, Cin: int, H: int, W: int) -> torch.Tensor:
    """dx [B, Cin, H, W] fp64 = F.conv_transpose2d(dy as NCHW, weight, stride 4).  dy [M, >= Cout] (row m = (b, i, j) patch-major, the
    first Cout columns count), w [Cout, >= Cin * 16] with column k = c*16 + kh*4 + kw (the conv weight [Cout, Cin, 4, 4] flattened)."""
    Cout = w.shape[0]
    g = dy[:, :Cout].double().cpu().reshape(B, H // 4, W // 4, Cout).permute(0, 3, 1, 2).contiguous()
    wt = w[:, : Cin * 16].double().cpu().reshape(Cout, Cin, 4, 4)
    return F.conv_transpose2d(g, wt, stride=4)


def col2im_ref(patches: torch.Tensor, B: int, Cin: int, H: int, W: int) -> torch.Tensor:
    """The inverse of the stem's im2col: patches [M, >= Cin * 16] -> [B, Cin, H, W] fp64."""
    p = patches[:, : Cin * 16].double().cpu().reshape(B, H // 4, W // 4, Cin, 4, 4)
    return p.permute(0, 3, 1, 4, 2, 5).reshape(B, Cin, H, W).contiguous()


def meta_input_grad_ref(heads, B: int, width: int, base=None) -> torch.Tensor:
    """dmeta [B, width] fp64: base (or zero) + for every (dp0 [B, C], w0 [C, >= dim], dim, off): dp0 @ w0[:, :dim] into columns off .. off + dim."""
    out = torch.zeros(B, width, dtype=torch.float64) if base is None else base.double().cpu().clone()
    for dp0, w0, dim, off in heads:
        out[:, off: off + dim] += dp0.double().cpu() @ w0[:, :dim].double().cpu()
    return out


def integer_probe(shape, lo: int, hi: int, seed: int) -> torch.Tensor:
    """Small integers (exact in bf16 and in any fp32 summation order at these sizes), fp32."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def asymmetric_weight(Cout: int, Cin: int, seed: int) -> torch.Tensor:
    """[Cout, 64] integer weight with no symmetry between rows, columns, taps or channels: entry (o, k) depends on o, c, kh and kw with
    different strides, so a swapped index cannot reproduce it.  Columns >= Cin * 16 (the arena's padding) hold a large value that must
    never reach dx."""
    w = torch.empty(Cout, 64)
    o = torch.arange(Cout).view(-1, 1)
    k = torch.arange(64).view(1, -1)
    c, kh, kw = k // 16, (k // 4) % 4, k % 4
    w[:] = ((o * 5 + c * 7 + kh * 3 + kw * 11 + seed) % 9 - 4).float()
    w[:, Cin * 16:] = 64.0
    return w
