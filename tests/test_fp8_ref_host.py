"""CPU tests of tests/fp8_ref.py: the references and the exact probe data the GPU tests of the fp8 / MXFP8 kernels rest on."""
import pytest
import torch

from tests import fp8_ref as R


def _all_finite_codes():
    b = torch.arange(256, dtype=torch.int32)
    return b[(b & 0x7F) != 0x7F].to(torch.uint8)


def test_every_e4m3_product_is_a_bf16_value():
    """What makes torch.equal the right comparison for the probes: the product of any two finite e4m3fn values has at most 8
    significant bits, so it survives the fp32 accumulator and the bf16 store unchanged."""
    v = R.e4m3_to_float(_all_finite_codes()).double()
    prod = v[:, None] * v[None, :]
    assert torch.equal(prod.float().double(), prod)
    assert torch.equal(prod.float().bfloat16().double(), prod)


@pytest.mark.parametrize("side", ["A", "W"])
@pytest.mark.parametrize("scales", ["mx", "pow2"])
@pytest.mark.parametrize("M,N,K", [(300, 80, 256), (130, 400, 384)])
def test_probe_expected_is_the_dense_product(M, N, K, side, scales):
    p = R.probe_operands(M, N, K, side, seed=M + N + K, scales=scales)
    A, W = p["Ad"].double(), p["Wd"].double()
    if scales == "mx":
        # Ad / Wd restated from the bytes and the PACKED scales: the layout the kernel streams
        ea, ew = R.unpack_scales(p["sa"]), R.unpack_scales(p["sw"])
        A = (R.e4m3_to_float(p["A8"]).double().view(M, K // 32, 32) * torch.exp2(ea.double() - 127).unsqueeze(-1)).view(M, K)
        W = (R.e4m3_to_float(p["W8"]).double().view(N, K // 32, 32) * torch.exp2(ew.double() - 127).unsqueeze(-1)).view(N, K)
        assert torch.equal(A.float(), p["Ad"]) and torch.equal(W.float(), p["Wd"])
        ref = A @ W.t()
    else:
        ref = (A @ W.t()) * (p["sa"].double() * p["sw"].double())
    assert p["expected"].dtype == torch.bfloat16 and p["expected"].shape == (M, N)
    assert torch.equal(p["expected"].double(), ref)   # one non-zero term per output: the fp64 sum is that term


@pytest.mark.parametrize("side", ["A", "W"])
def test_probe_with_arbitrary_scales_restates_two_roundings(side):
    M, N, K = 300, 80, 256
    p = R.probe_operands(M, N, K, side, seed=5, scales="arbitrary")
    prod32 = (p["Ad"].double() @ p["Wd"].double().t()).float()            # exact
    assert torch.equal(p["expected"], (prod32 * (p["sa"] * p["sw"])).bfloat16())
    # ... which is the fp64 product to within the fp32 rounding plus the bf16 rounding
    ref = prod32.double() * p["sa"].double() * p["sw"].double()
    assert ((p["expected"].double() - ref).abs() <= ref.abs() * (2.0 ** -8 + 2.0 ** -22)).all()


@pytest.mark.parametrize("side", ["A", "W"])
@pytest.mark.parametrize("scales", ["mx", "pow2", "arbitrary"])
def test_probe_bytes_are_normal_codes_and_cover_every_k(side, scales):
    M, N, K = 400, 400, 384
    p = R.probe_operands(M, N, K, side, seed=9, scales=scales)
    hot, dense = (p["A8"], p["W8"]) if side == "A" else (p["W8"], p["A8"])
    for t in (hot, dense):
        mag = t & 0x7F
        assert not (mag == 0x7F).any()                    # 0x7f / 0xff: NaN
        assert not ((mag > 0) & (mag < 0x08)).any()       # subnormals
    assert not (dense & 0x7F == 0).any()
    assert (dense >= 0x80).any() and (dense < 0x80).any() and (hot >= 0x80).any()
    nz = hot != 0
    assert (nz.sum(1) == 1).all()
    rows = torch.arange(hot.shape[0])
    assert nz[rows, (37 * rows + 11) % K].all()
    assert nz.any(0).all()                                # at least K rows: every k position is probed
    if scales == "mx":
        for e in (p["ea"], p["ew"]):
            assert e.min() >= 119 and e.max() <= 135 and len(e.unique()) == 17
    # seeded: the same call gives the same bytes
    q = R.probe_operands(M, N, K, side, seed=9, scales=scales)
    assert torch.equal(q["A8"], p["A8"]) and torch.equal(q["W8"], p["W8"]) and torch.equal(q["expected"], p["expected"])


def test_probe_positions_are_a_permutation_for_every_k_in_use():
    for K in (256, 384, 512, 640, 896, 1152, 1536):
        assert len(R.probe_positions(K, K).unique()) == K


def test_pack_unpack_round_trip():
    e = torch.arange(7 * 12, dtype=torch.int32).reshape(7, 12).to(torch.uint8)
    sc = R.pack_scales(e)
    assert sc.shape == (3, 7, 4) and sc.is_contiguous()
    for r, kb in ((0, 0), (3, 5), (6, 11)):
        assert sc[kb // 4, r, kb % 4] == e[r, kb]         # byte kb & 3 of dword [kb >> 2][row]
    assert torch.equal(R.unpack_scales(sc), e)
    assert torch.equal(R.pack_scales(R.unpack_scales(sc)), sc)


def _bytes(q):
    return q.view(torch.uint8)


def test_mx_reference_on_hand_computed_blocks():
    x = torch.zeros(6, 32)
    # row 0: amax = 1.75 * 2^3 = 14 sits ON the boundary: 14 * 2^-(3 - 8) = 448 fits, so e = 3 - 8 + 127 = 122, elements x * 32
    x[0, 0], x[0, 1], x[0, 2] = 14.0, -1.0, 0.5
    # row 1: one fp32 ulp above the boundary: the next scale, e = 123, elements x * 16
    x[1, 0], x[1, 1] = torch.tensor(14.0).nextafter(torch.tensor(100.0)), -1.0
    # row 2: the zero block: the smallest scale, E8M0 0, zero bytes
    # row 3: amax = 1.0 = 1.0 * 2^0 -> e = 119, elements x * 256
    x[3, 0], x[3, 5] = 1.0, -0.75
    # row 4: rounding to nearest even inside a block: amax 448 -> e = 127 (scale 1); 17 lies between 16 and 18 -> 16 (even mantissa),
    # 19 lies between 18 and 20 -> 20, 21 -> 20 (between 20 and 22: mantissa 010 is even)
    x[4, 0], x[4, 1], x[4, 2], x[4, 3] = 448.0, 17.0, 19.0, -21.0
    # row 5: the top of the fp32 range: e = 127 + 127 - 8 + 1 = 247 <= 254, amax 3e38 = 1.763 * 2^127 -> just past 1.75
    x[5, 0] = 3e38
    q, e = R.mx_reference(x)
    qb, qf = _bytes(q), q.float()
    assert e[:, 0].tolist() == [122, 123, 0, 119, 127, 247]
    assert qb[0, 0] == 0x7E and qf[0, 1] == -32.0 and qf[0, 2] == 16.0          # 0x7e = 448: the largest finite code
    assert qf[1, 0] == 224.0 and qf[1, 1] == -16.0
    assert not qb[2].any()
    assert qf[3, 0] == 256.0 and qf[3, 5] == -192.0
    assert qf[4, :4].tolist() == [448.0, 16.0, 20.0, -20.0]
    assert qf[5, 0] == 224.0                                                     # 3e38 * 2^-120 = 225.7
    assert not ((qb & 0x7F) == 0x7F).any()


def test_fp8_reference_on_hand_computed_values():
    x = torch.tensor([[448.0, -448.0, 224.0, 17.0, 19.0, 0.0, 1000.0, -1e30]])
    q, s = R.fp8_reference(x, torch.tensor([448.0]))      # inv = 1
    assert s.item() == 1.0
    assert q.float()[0].tolist() == [448.0, -448.0, 224.0, 16.0, 20.0, 0.0, 448.0, -448.0]   # ties to even; saturation
    assert _bytes(q)[0, 6] == 0x7E and _bytes(q)[0, 7] == 0xFE
    # delayed scaling: amax = half the maximum -> inv = 2, everything beyond +-224 saturates to +-448, never to the NaN code
    q, s = R.fp8_reference(x, torch.tensor([224.0]))
    assert s.item() == 0.5
    assert q.float()[0].tolist() == [448.0, -448.0, 448.0, 32.0, 40.0, 0.0, 448.0, -448.0]   # (34 -> 32 and 38 -> 40: ties to even)
    assert not ((_bytes(q) & 0x7F) == 0x7F).any()
    # a quotient that is not a power of two: 448 / 3 rounded to fp32 once
    q, s = R.fp8_reference(torch.tensor([[3.0, 1.0]]), 3.0)
    inv = torch.tensor(448.0 / 3.0, dtype=torch.float32)
    assert s.item() == torch.tensor(3.0 / 448.0, dtype=torch.float32).item()
    assert q.float()[0].tolist() == [448.0, (torch.tensor(1.0) * inv).to(torch.float8_e4m3fn).float().item()]
    # the all-zero tensor: scale 1, zero bytes
    q, s = R.fp8_reference(torch.zeros(2, 16), 0.0)
    assert s.item() == 1.0 and not _bytes(q).any()
