"""Definitions the fp8 / MXFP8 tests compare against (csrc/gemm_fp8.hip), in plain torch on whatever device holds the tensors.

mx_reference / fp8_reference restate the two quantisers.  pack_scales / unpack_scales convert between one E8M0 byte per (row,
32-element block) and the layout the GEMM streams, [K/128][rows][4].  probe_operands builds EXACT probe data for the GEMMs: bytes and
scales written directly (no quantiser involved), one operand with a single non-zero per row, so that every output element is one product
a * 2^ea * w * 2^ew.  An e4m3 x e4m3 product has at most 8 significant bits (two 4-bit significands; checked over all finite code pairs
by tests/test_fp8_ref_host.py), so with power-of-two scales it is a bf16 value and the kernel's output must equal it bit for bit.
"""
import torch

E4M3_MAX = 448.0
PROBE_STEP, PROBE_OFF = 37, 11            # the non-zero of row r sits at k = (37 r + 11) % K; 37 is coprime to every multiple of 128
SCALE_LO, SCALE_HI = 119, 135             # probe block scales 2^-8 .. 2^8 (E8M0, bias 127)
BF16_MIN_NORMAL = 2.0 ** -126
BF16_MAX = 3.3895313892515355e38


def mx_reference(x):
    """The definition lnx_quantize_mxfp8 implements, restated with torch integer ops: per 32-element block the smallest
    power of two 2^e with amax * 2^-e <= 448, elements = e4m3fn(x * 2^-e) (torch's round-to-nearest-even conversion)."""
    M, K = x.shape
    xb = x.float().view(M, K // 32, 32)
    bits = xb.abs().amax(-1).contiguous().view(torch.int32)
    e = ((bits >> 23) & 0xFF) - 8 + ((bits & 0x7FFFFF) > 0x600000).int()
    e = e.clamp(0, 254)
    inv = ((254 - e) << 23).view(torch.float32)
    q = (xb * inv.unsqueeze(-1)).clamp(-448, 448).to(torch.float8_e4m3fn).view(M, K)
    return q, e.to(torch.uint8)  # e: [M, K/32]


def fp8_reference(x, amax):
    """The definition lnx_quantize_fp8 implements: one fp32 multiply by the correctly rounded fp32 value of 448 / amax, a clamp to
    +-448 and torch's round-to-nearest-even e4m3fn conversion; scale = the correctly rounded fp32 value of amax / 448.  (Both
    quotients through Python doubles: a tensor division on the GPU may be a reciprocal-multiply, one ulp off.)  amax = 0 gives scale 1.
    Returns (bytes as torch.float8_e4m3fn, scale as a 1-element fp32 tensor on x's device)."""
    am = float(torch.as_tensor(amax, dtype=torch.float32).reshape(-1)[0].item())
    inv = torch.tensor(E4M3_MAX / am if am > 0 else 1.0, dtype=torch.float32).item()
    scale = torch.tensor([am / E4M3_MAX if am > 0 else 1.0], dtype=torch.float32, device=x.device)
    q = (x.float() * inv).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    return q, scale


def pack_scales(e):
    """[rows, K/32] uint8 -> the streamed layout [K/128, rows, 4]: byte j of [ks, r] = block 4 ks + j of row r."""
    rows, nb = e.shape
    assert nb % 4 == 0
    return e.view(rows, nb // 4, 4).permute(1, 0, 2).contiguous()


def unpack_scales(sc):
    """[K/128, rows, 4] -> [rows, K/32]."""
    ks, rows, four = sc.shape
    assert four == 4
    return sc.permute(1, 0, 2).reshape(rows, ks * 4)


def e4m3_to_float(b):
    """uint8 e4m3fn codes -> their fp32 values (exact)."""
    return b.view(torch.float8_e4m3fn).float()


def _normal_codes(shape, gen, device):
    """Random NORMAL e4m3fn codes of both signs: magnitude bytes 0x08 .. 0x7e (no zero, no subnormal 0x01..0x07, no NaN 0x7f)."""
    mag = torch.randint(0x08, 0x7F, shape, generator=gen, device=device, dtype=torch.int32)
    sign = torch.randint(0, 2, shape, generator=gen, device=device, dtype=torch.int32) << 7
    return (mag | sign).to(torch.uint8)


def probe_positions(rows, K, device="cpu"):
    return (PROBE_STEP * torch.arange(rows, device=device, dtype=torch.int64) + PROBE_OFF) % K


def probe_operands(M, N, K, side, seed, *, scales="mx", device="cpu"):
    """Exact probe data for out = A . W^T at (M, N, K).

    side = "A": A8 has one non-zero per row, at k = (37 m + 11) % K, and W8 is dense; side = "W": the mirror image.  Every byte is a
    normal e4m3fn code of either sign.  scales = "mx": random E8M0 bytes in [119, 135] per (row, 32-block) for both operands;
    "pow2": per-tensor scales 2^-3 and 2^5; "arbitrary": per-tensor scales 0.7391 and 1.2873 as fp32.

    Returns a dict: A8, W8 (uint8 [M, K], [N, K]); for "mx" ea, ew (uint8 [rows, K/32]) and sa, sw in the streamed layout
    [K/128, rows, 4]; otherwise sa, sw as 1-element fp32 tensors; Ad, Wd = the fp32 values the operands stand for WITHOUT the
    per-tensor scales (with the block scales for "mx"); expected = the bf16 output.  Every expected value is the single product
    a 2^ea w 2^ew, exact in fp32 and in bf16; for "arbitrary" it restates the kernel's two roundings, bf16(fp32(a w) * fp32(sa sw))."""
    assert side in ("A", "W") and scales in ("mx", "pow2", "arbitrary") and K % 128 == 0
    gen = torch.Generator(device=device).manual_seed(seed)
    hot_rows, dense_rows = (M, N) if side == "A" else (N, M)
    pos = probe_positions(hot_rows, K, device)
    hot = torch.zeros(hot_rows, K, dtype=torch.uint8, device=device)
    hot_val = _normal_codes((hot_rows,), gen, device)
    hot[torch.arange(hot_rows, device=device), pos] = hot_val
    dense = _normal_codes((dense_rows, K), gen, device)
    A8, W8 = (hot, dense) if side == "A" else (dense, hot)
    out = {"A8": A8, "W8": W8}
    Ad, Wd = e4m3_to_float(A8), e4m3_to_float(W8)
    if scales == "mx":
        ea = torch.randint(SCALE_LO, SCALE_HI + 1, (M, K // 32), generator=gen, device=device, dtype=torch.int32).to(torch.uint8)
        ew = torch.randint(SCALE_LO, SCALE_HI + 1, (N, K // 32), generator=gen, device=device, dtype=torch.int32).to(torch.uint8)
        Ad = (Ad.view(M, K // 32, 32) * torch.exp2(ea.float() - 127.0).unsqueeze(-1)).view(M, K)
        Wd = (Wd.view(N, K // 32, 32) * torch.exp2(ew.float() - 127.0).unsqueeze(-1)).view(N, K)
        out.update(ea=ea, ew=ew, sa=pack_scales(ea), sw=pack_scales(ew))
        alpha = None
    else:
        sa, sw = (2.0 ** -3, 2.0 ** 5) if scales == "pow2" else (0.7391, 1.2873)
        out.update(sa=torch.tensor([sa], dtype=torch.float32, device=device), sw=torch.tensor([sw], dtype=torch.float32, device=device))
        alpha = out["sa"] * out["sw"]  # one fp32 multiply, as the kernel's
    # the one product per output, in fp32 (exact: 8 significant bits, exponents far inside the fp32 range)
    if side == "A":
        exp32 = Ad[torch.arange(M, device=device), pos].unsqueeze(1) * Wd[:, pos].t()
    else:
        exp32 = Ad[:, pos] * Wd[torch.arange(N, device=device), pos].unsqueeze(0)
    if alpha is not None:
        exp32 = exp32 * alpha
    mag = exp32.abs()
    assert torch.isfinite(exp32).all() and (mag >= BF16_MIN_NORMAL).all() and (mag <= BF16_MAX).all(), "probe product outside bf16's normal range"
    expected = exp32.bfloat16()
    if scales != "arbitrary":
        assert torch.equal(expected.float(), exp32), "probe product is not a bf16 value"
    out.update(Ad=Ad, Wd=Wd, expected=expected)
    return out
