"""fp64 restatement of the rotate mode of the RoPE attention (MODEL.ROPE_STAGES.ROPE_ROTATE, LNX_ROPE_ROTATE): the tables, the
rotated attention forward, and a hand-written backward including the gradient of the learnable frequencies.

    theta[n,h,j] = t_x freqs[0,h,j] + t_y freqs[1,h,j],  t_x = n % W, t_y = n // W         (image tokens only)
    x'[2j]   = x[2j] cos(theta) - x[2j+1] sin(theta)
    x'[2j+1] = x[2j] sin(theta) + x[2j+1] cos(theta)                                        x in {q, k}
    q' *= D^-0.5;  P = softmax(q' k'^T) [* drop];  o = P v
    dx[2j]   =  dx'[2j] cos + dx'[2j+1] sin,   dx[2j+1] = -dx'[2j] sin + dx'[2j+1] cos
    dtheta   = sum_b sum_{x in {q,k}} (dx'[2j+1] x'[2j] - dx'[2j] x'[2j+1])
    dfreqs[0] = sum_n t_x dtheta,  dfreqs[1] = sum_n t_y dtheta

Plain real arithmetic on torch fp64 tensors: no complex numbers, no autograd, nothing shared with the kernels.  tests/test_rope_rotate.py
pins it to the reference's compute_mixed_cis / apply_rotary_emb (recorded by tests/golden/gen/make_golden_rope_rotate.py) and to
torch's fp64 autograd through complex operations."""
import torch


def grid(H, W):
    n = torch.arange(H * W, dtype=torch.float64)
    return n % W, torch.div(n, W, rounding_mode="floor")


def tables(freqs, H, W):
    """(cos(theta), sin(theta)), each [H W, heads, D/2], of freqs [2, heads, D/2]"""
    tx, ty = grid(H, W)
    theta = tx[:, None, None] * freqs[0].double()[None] + ty[:, None, None] * freqs[1].double()[None]
    return torch.cos(theta), torch.sin(theta)


def rotate(x, cos, sin):
    """x [B, heads, H W, D] -> x'; cos / sin [H W, heads, D/2]"""
    c, s = cos.permute(1, 0, 2)[None], sin.permute(1, 0, 2)[None]
    e, o = x[..., 0::2], x[..., 1::2]
    return torch.stack([e * c - o * s, e * s + o * c], -1).flatten(-2)


def rotate_bwd(dxp, cos, sin):
    """gradient of x given the gradient of x' = rotate(x): the inverse rotation"""
    c, s = cos.permute(1, 0, 2)[None], sin.permute(1, 0, 2)[None]
    e, o = dxp[..., 0::2], dxp[..., 1::2]
    return torch.stack([e * c + o * s, -e * s + o * c], -1).flatten(-2)


def dtheta_of(dxp, xp):
    """[H W, heads, D/2]: sum over the batch of dx'[2j+1] x'[2j] - dx'[2j] x'[2j+1]; xp, dxp [B, heads, H W, D]"""
    return (dxp[..., 1::2] * xp[..., 0::2] - dxp[..., 0::2] * xp[..., 1::2]).sum(0).permute(1, 0, 2)


def dfreqs_of(dtheta, H, W):
    tx, ty = grid(H, W)
    return torch.stack([(tx[:, None, None] * dtheta).sum(0), (ty[:, None, None] * dtheta).sum(0)])


def _split(qkv, B, N, heads, hd):
    t = qkv.double().reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def attn_fwd(qkv, freqs, B, N, E, heads, hd, H, W, drop=None, rotate_mode=True):
    """o [B N, heads hd] and what the backward needs.  qkv [B N, 3 heads hd]; drop: optional multiplier [B, heads, N, N] of the
    normalised probabilities.  rotate_mode False: the cos-only form (the real part of the same table)."""
    q, k, v = _split(qkv, B, N, heads, hd)
    if N > E:
        cos, sin = tables(freqs, H, W)
        if not rotate_mode:
            sin = torch.zeros_like(sin)
            qi, ki = q[:, :, E:] * cos.permute(1, 0, 2)[None].repeat_interleave(2, -1), k[:, :, E:] * cos.permute(1, 0, 2)[None].repeat_interleave(2, -1)
        else:
            qi, ki = rotate(q[:, :, E:], cos, sin), rotate(k[:, :, E:], cos, sin)
        qp, kp = torch.cat([q[:, :, :E], qi], 2), torch.cat([k[:, :, :E], ki], 2)
    else:
        cos = sin = None
        qp, kp = q, k
    qp = qp * hd ** -0.5
    p = torch.softmax(qp @ kp.transpose(-2, -1), -1)
    pd = p if drop is None else p * drop.double()
    o = (pd @ v).transpose(1, 2).reshape(B * N, heads * hd)
    return o, dict(qp=qp, kp=kp, v=v, p=p, drop=drop, cos=cos, sin=sin)


def attn_bwd(d_o, saved, B, N, E, heads, hd, H, W):
    """(dqkv [B N, 3 heads hd], dfreqs [2, heads, hd/2] or None) of the rotate-mode forward that produced `saved`"""
    qp, kp, v, p, drop = saved["qp"], saved["kp"], saved["v"], saved["p"], saved["drop"]
    do = d_o.double().reshape(B, N, heads, hd).transpose(1, 2)
    pd = p if drop is None else p * drop.double()
    dv = pd.transpose(-2, -1) @ do
    dpd = do @ v.transpose(-2, -1)
    dp = dpd if drop is None else dpd * drop.double()
    ds = p * (dp - (dp * p).sum(-1, keepdim=True))
    dqp = ds @ kp            # gradient of the scaled, rotated q
    dkp = ds.transpose(-2, -1) @ qp
    dq, dk = dqp * hd ** -0.5, dkp.clone()
    dfreqs = None
    if N > E:
        cos, sin = saved["cos"], saved["sin"]
        dth = dtheta_of(dqp[:, :, E:], qp[:, :, E:]) + dtheta_of(dkp[:, :, E:], kp[:, :, E:])  # x' and dx' both after q's scale
        dfreqs = dfreqs_of(dth, H, W)
        dq = torch.cat([dq[:, :, :E], rotate_bwd(dq[:, :, E:], cos, sin)], 2)
        dk = torch.cat([dk[:, :, :E], rotate_bwd(dk[:, :, E:], cos, sin)], 2)
    dqkv = torch.stack([dq, dk, dv]).permute(1, 3, 0, 2, 4).reshape(B * N, 3 * heads * hd)
    return dqkv, dfreqs
