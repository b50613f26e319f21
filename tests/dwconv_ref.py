"""Plain fp64 restatement of the depthwise 7x7 convolution (padding 3, NHWC) and of its three gradients, with no library convolution:
zero-pad by 3, then 49 shifted slices times the tap.  Works on any device (the GPU tests run it on the device; tests/test_dwconv_ref.py
pins it to oracle.mformer_oracle.depthwise_conv7 + autograd and to the recorded reference output on the CPU).

Also the launch arithmetic of the three kernel families (csrc/dwconv.hip, csrc/dwconv_mfma.hip), restated so that a test can assert how
long the walks of a case are on the device it runs on."""
import torch


def dwconv7_ref(x, w, bias=None, dy=None):
    """x [B, H, W, C], w [C, 7, 7] (or [C, 1, 7, 7]), bias [C] or None, dy [B, H, W, C] or None; any floating dtype, computed in fp64.
    Returns (y, dx, dw, db): y[b, h, w, c] = bias[c] + sum_{ky, kx} w[c, ky, kx] x[b, h + ky - 3, w + kx - 3, c] (zero outside the
    image) and, with dy, the gradients of sum(y * dy): dx [B, H, W, C], dw [C, 7, 7], db [C] (None without dy)."""
    B, H, W, C = x.shape
    w = w.reshape(C, 7, 7).double()
    xp = torch.zeros(B, H + 6, W + 6, C, dtype=torch.float64, device=x.device)
    xp[:, 3:H + 3, 3:W + 3] = x
    y = torch.zeros(B, H, W, C, dtype=torch.float64, device=x.device)
    dxp = dw = db = None
    if dy is not None:
        dy = dy.double()
        dxp = torch.zeros_like(xp)
        dw = torch.zeros(C, 7, 7, dtype=torch.float64, device=x.device)
        db = dy.sum((0, 1, 2))
    for ky in range(7):
        for kx in range(7):
            window = xp[:, ky:ky + H, kx:kx + W]
            y += window * w[:, ky, kx]
            if dy is not None:
                dxp[:, ky:ky + H, kx:kx + W] += dy * w[:, ky, kx]
                dw[:, ky, kx] = (window * dy).sum((0, 1, 2))
    if bias is not None:
        y += bias.double()
    return y, (None if dy is None else dxp[:, 3:H + 3, 3:W + 3].contiguous()), dw, db


def cdiv(a, b):
    return -(-a // b)


def launch_cus(device_cus, margin):
    """dwconv_mfma.hip cus(): the device's compute units (256 if unknown) minus the margin, at least 8"""
    return max(8, (device_cus if device_cus > 0 else 256) - margin)


def mfma_fwd_walk(B, H, W, C, cus):
    """lnx_dwconv7_mfma_fwd: 14x14 tiles numbered row-major over (image, tile row, tile column); a workgroup owns one 32-channel block
    and tiles [i * per, min(ntile, (i + 1) * per)).  Returns dict(ntile, per, chunks, tiles_h, tiles_w)."""
    th, tw = cdiv(H, 14), cdiv(W, 14)
    ntile = B * th * tw
    chunks = min(max(cus // (C // 32), 1), ntile)
    per = cdiv(ntile, chunks)
    return dict(ntile=ntile, per=per, chunks=cdiv(ntile, per), tiles_h=th, tiles_w=tw)


def mfma_wgrad_walk(B, H, W, C, cus):
    """lnx_dwconv7_mfma_wgrad: 14x28 tiles, `walkers` contiguous runs of `per` tiles for each of the C / 32 groups, two 16-channel
    sibling workgroups per (walker, group) pair, grid = 16 * ceil(walkers * groups / 8)"""
    th, tw = cdiv(H, 14), cdiv(W, 28)
    ntile, groups = B * th * tw, C // 32
    walkers = min(max(cus // groups, 1), ntile)
    per = cdiv(ntile, walkers)
    walkers = cdiv(ntile, per)
    return dict(ntile=ntile, per=per, walkers=walkers, groups=groups, pairs=walkers * groups, grid=16 * cdiv(walkers * groups, 8), tiles_h=th, tiles_w=tw)


def valu_fwd_walk(B, H, W, C):
    """lnx_dwconv7_fwd (VALU): 8x16 tiles, a walk of one image's tiles halved until there are 768 workgroups; the margin plays no part"""
    th, tw = cdiv(H, 8), cdiv(W, 16)
    ntile, cblocks = B * th * tw, C // 32
    per = th * tw
    while per > 1 and cdiv(ntile, per) * cblocks < 768:
        per = (per + 1) // 2
    return dict(ntile=ntile, per=per, chunks=cdiv(ntile, per), tiles_h=th, tiles_w=tw)


def valu_wgrad_walk(B, H, W, C):
    """lnx_dwconv7_wgrad (VALU): min(768 / cblocks, ntile) walkers per channel block, walker i takes tiles i, i + walkers, ..."""
    th, tw = cdiv(H, 8), cdiv(W, 16)
    ntile = B * th * tw
    walkers = min(max(768 // (C // 32), 1), ntile)
    return dict(ntile=ntile, per=cdiv(ntile, walkers), walkers=walkers, tiles_h=th, tiles_w=tw)


def walk_crossings(ntile, per, tiles_h, tiles_w):
    """what the contiguous walks [i * per, (i + 1) * per) of a row-major tile numbering meet: (a walk spans two tile rows of one image,
    a walk spans two images, the last walk is shorter than the others)"""
    row = image = False
    for t0 in range(0, ntile, per):
        t1 = min(ntile, t0 + per) - 1
        if t0 // (tiles_h * tiles_w) != t1 // (tiles_h * tiles_w):
            image = True
        for t in range(t0, t1):  # consecutive tiles t, t + 1 of one walk in one image but in different tile rows
            if t // (tiles_h * tiles_w) == (t + 1) // (tiles_h * tiles_w) and t // tiles_w != (t + 1) // tiles_w:
                row = True
    return row, image, ntile % per != 0
