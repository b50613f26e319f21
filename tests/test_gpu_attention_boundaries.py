"""lnx_attn_fwd / lnx_attn_bwd at every sequence-length seam of every kernel family (resident 4 / 8 waves, tiled 64- / 128-row tiles):
N = 0, 1, 32, 33 (mod 64), 64 / 65, 128 / 129, 256 / 257, multiples of 128 and the production lengths 260, 788, 1028, at head_dim 32,
64 and 128 in fp32 and bf16, with B = 2 and 2 heads so that another sample and another head lie behind every row a clamped or
unmasked access could reach.  Each case asserts the family that ran (lnx_last_attn_kernel) against a literal table.

Two kinds of check:
 * test_sweep_*: against the fp64 restatement attn_ref of test_gpu_headdim.py with that file's tolerances (forward 3e-5 / 2e-2,
   dqkv and dfreqs 1e-4 / 4e-2 for fp32 / bf16);
 * test_nothing_outside_the_sequence_matters: no tolerance.  Every buffer carries G = 130 guard rows; the outputs of sample 0 must
   not change by one bit when sample 1 and every guard go from ordinary values to |x| = 1e3, nor when the dropout mask's padding
   columns and guard rows are flipped, and no guard may be written.

Why the second kind: what one phantom key does to the forward output, in fp64 on the CPU (B = heads = 2, head_dim 64, standard
normal q / k / v; share of output elements outside atol + rtol |o|, and the largest error against the largest |o|):

     N | extra key                  | outside 2e-2 | outside 3e-5 | max err / max |o|
    65 | all-zero key / value row   |      0.00 %  |     98.59 %  | 9.8e-03 / 1.60
    65 | the next sample's row 0    |     16.48 %  |     99.48 %  | 2.8e-01 / 1.60
   129 | all-zero key / value row   |      0.00 %  |     96.31 %  | 3.0e-03 / 0.65
   129 | the next sample's row 0    |      4.62 %  |     98.94 %  | 1.6e-01 / 0.65
   257 | all-zero key / value row   |      0.00 %  |     90.00 %  | 1.4e-03 / 0.60
   257 | the next sample's row 0    |      1.20 %  |     98.73 %  | 1.6e-01 / 0.60
   513 | all-zero key / value row   |      0.00 %  |     71.96 %  | 4.1e-04 / 0.43
   513 | the next sample's row 0    |      0.24 %  |     96.85 %  | 7.4e-02 / 0.43

The bf16 tolerance never sees a zero padding key let into the softmax, and sees a neighbour's row in a shrinking share of the
elements; the fp32 tolerance sees both.  The bit-exact checks see any read that reaches a result, in either dtype.  Padding the
kernels make themselves (zeroed or clamped LDS rows) is out of their reach, and the resident and 128-row kernels have no fp32
twin, so test_forward_where_a_padding_key_would_decide runs the forward on inputs where such a key would be the whole answer.

Which case fails if a seam were off by one (from the code, csrc/attention.hip):
 * resident forward, `p.N - nf * BT > 32` (64 or 32 keys in the last step): with `> 33` a last tile of 33 live keys takes the
   32-key step and loses key N - 1, a real key of weight about 1 / 33 at N = 33: test_sweep_against_fp64[bf16-64-N33-...] (and N97,
   N193), and test_forward_where_a_padding_key_would_decide[bf16-64-33], where the lost key is the 64-fold row of v;
 * tiled key mask, `key < p.N` in the last key tile: with `<=` key N (a clamped copy of key N - 1, or for a neighbour-reading
   variant sample 1's row 0) enters the softmax: test_sweep_against_fp64[fp32-*-N65-...] and every other N not a multiple of 64
   at 3e-5, test_forward_where_a_padding_key_would_decide[bf16-*] for the 128-row kernels fp32 never runs, and
   test_nothing_outside_the_sequence_matters if the extra row comes from memory;
 * 128-row tiling, `qtiles = cdiv(N, 128)`: with N / 128 the rows of the last partial tile are never computed, so o / dqkv / lse /
   delta keep their NaN prefill at N = 129, 257, 260, 1028 (launch() refuses a NaN in any of them); with one tile too many the
   workgroup's stores land in sample 1 or the guard rows (bit-compared), and reduce_freqs folds a partial nobody wrote, which the
   dfreqs comparison of the sweep sees."""
import os
import re
import subprocess
import sys

import pytest
import torch

from linnaeus_amd import _lib as L
from linnaeus_amd import ops
from oracle import mformer_oracle as O
from tests.test_gpu_headdim import attn_ref

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {L.F32: torch.float32, L.BF16: torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.uint8: torch.uint8}
DTN = {L.F32: "fp32", L.BF16: "bf16"}
B, HEADS, G, RATE = 2, 2, 130, 0.25
R4, R8, T4, T8 = L.ATTN_KERNEL_RES4, L.ATTN_KERNEL_RES8, L.ATTN_KERNEL_TILED4, L.ATTN_KERNEL_TILED8

NS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 191, 192, 193, 255, 256, 257,
      260, 319, 320, 321, 383, 384, 385, 511, 512, 513, 788, 1028]
THIN = [32, 33, 64, 65, 128, 129, 192, 256, 257, 260]
DEGENERATE = [64, 128, 256, 257]  # also E = 0 (image tokens only) and E = N (no image tokens, no tables)


def grid(M):
    """M = H * W with H < W and H as large as it gets (1 x M for a prime), so that a transposed table cannot pass"""
    if M == 1:
        return 1, 1
    h = max(d for d in range(1, int(M ** 0.5) + 1) if M % d == 0 and d * d != M)
    return h, M // h


def split(N, i):
    """(H, W, E) with H * W + E = N: E from {3, 4, 1} (the first choice rotates with i), preferring an E whose image grid has two
    real sides; N = 1 has no image token"""
    if N == 1:
        return 0, 0, 1
    order = [(3, 4, 1)[(i + j) % 3] for j in range(3)]
    fits = [E for E in order if N - E >= 1]
    two_sided = [E for E in fits if grid(N - E)[0] > 1]
    E = (two_sided or fits)[0]
    H, W = grid(N - E)
    return (W, H, E) if i % 2 and H > 1 else (H, W, E)  # both orientations over the list


PRIMARY = {N: (N,) + split(N, i) for i, N in enumerate(NS)}
CASES = list(PRIMARY.values())
for N in DEGENERATE:
    CASES += [(N,) + grid(N) + (0,), (N, 0, 0, N)]
THIN_CASES = [PRIMARY[N] for N in THIN]
assert {c[0] for c in CASES} == set(NS) and len(PRIMARY) == len(NS) == 36, "a listed length lost its case"
assert all(H * W + E == N and (H * W == 0 or H != W or H == 1) for N, H, W, E in CASES)
assert {c[3] for c in CASES} >= {0, 1, 3, 4}

# dtype, head_dim -> (largest N, family) in rising order; lnx_attn_dispatch's table (include/lnx.h) as literals
FAMILY = {
    (L.F32, 32): [(1 << 30, T4)], (L.F32, 64): [(1 << 30, T4)], (L.F32, 128): [(1 << 30, T4)],
    (L.BF16, 32): [(1 << 30, T4)],
    (L.BF16, 64): [(64, R4), (256, R8), (1 << 30, T8)],
    (L.BF16, 128): [(128, T4), (1 << 30, T8)],
}
FAMILY_TILED_SWITCH = {(L.BF16, 64): [(128, T4), (1 << 30, T8)]}                          # LNX_ATTN_TILED=1
FAMILY_NW4 = {(L.BF16, 64): [(64, R4), (256, R8), (1 << 30, T4)], (L.BF16, 128): [(1 << 30, T4)]}  # LNX_ATTN_NW=4
FAMILY_DROP = {k: [(1 << 30, T4)] for k in FAMILY}


def family_of(table, dtype, hd, N):
    return next(f for top, f in table[(dtype, hd)] if N <= top)


def case_id(c):
    return "N%d-%dx%d+%d" % c


def bits(t):
    return t.contiguous().view(BITS[t.dtype])


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def make_inputs(dtype, hd, case, drop, batch=B):
    N, H, W, E = case
    C_ = HEADS * hd
    gen = torch.Generator().manual_seed(1000 * N + hd + 7 * E + dtype)
    inp = dict(dtype=dtype, hd=hd, N=N, H=H, W=W, E=E, B=batch,
               qkv=torch.randn(batch * N, 3 * C_, generator=gen).to(DT[dtype]),
               d_o=torch.randn(batch * N, C_, generator=gen).to(DT[dtype]),
               freqs=O.seeded_fill("t.attn.freqs", (2, HEADS, hd // 2), 7), mask=None)
    if drop:
        Np = (N + 63) // 64 * 64
        inp["mask"] = (torch.rand(batch, HEADS, N, Np, generator=gen) >= RATE).to(torch.uint8)  # random in the padding columns too
    return inp


def big_like(t, gen):
    """|x| = 1e3 with random signs: finite, so that a legitimately zeroed probability times a loaded row stays 0"""
    return (torch.where(torch.rand(t.shape, generator=gen) < 0.5, -1e3, 1e3)).to(t.dtype)


def with_big_second_sample(inp):
    out = dict(inp)
    gen = torch.Generator().manual_seed(99)
    n = inp["N"]
    for k in ("qkv", "d_o"):
        out[k] = inp[k].clone()
        out[k][n:] = big_like(out[k][n:], gen)
    return out


def with_flipped_mask_padding(inp):
    out = dict(inp)
    out["mask"] = inp["mask"].clone()
    out["mask"][..., inp["N"]:] ^= 1
    return out


def launch(inp, guard=0, big=False, flip_mask_guard=False):
    """forward + backward on views of buffers that carry `guard` more rows (floats for lse / delta).  The guards hold ordinary random
    values, or |x| = 1e3 with big; they are outputs' sentinels too and are compared bit for bit after the calls.  Returns the CPU copies
    of o, lse, dqkv, delta, dfreqs and the family the library recorded."""
    dtype, hd, N, H, W, E, nb = (inp[k] for k in ("dtype", "hd", "N", "H", "W", "E", "B"))
    C_, half, rows, HW = HEADS * hd, hd // 2, inp["B"] * inp["N"], inp["H"] * inp["W"]
    gen = torch.Generator().manual_seed(4242)

    def guard_vals(shape, dt, unit=False):
        r = torch.rand(shape, generator=gen) * 2 - 1 if unit else torch.randn(shape, generator=gen)
        return (big_like(r, gen) if big else r).to(dt)

    def rows_buf(body, ncols, dt):  # [n + guard, ncols]: body (a CPU tensor or None = NaN, to be written) and the guard rows
        n = rows if body is None else body.shape[0]
        t = torch.full((n + guard, ncols), float("nan"), dtype=dt)
        if body is not None:
            t[:n] = body
        t[n:] = guard_vals((guard, ncols), dt)
        t = t.cuda()
        return t, t[:n]

    def flat_buf(n):  # n + guard floats, NaN then the guard
        t = torch.cat([torch.full((n,), float("nan")), guard_vals((guard,), torch.float32)]).cuda()
        return t, t[:n].view(nb, HEADS, N)

    qkv_b, qkv = rows_buf(inp["qkv"], 3 * C_, DT[dtype])
    do_b, d_o = rows_buf(inp["d_o"], C_, DT[dtype])
    o_b, o = rows_buf(None, C_, DT[dtype])
    dqkv_b, dqkv = rows_buf(None, 3 * C_, DT[dtype])
    lse_b, lse = flat_buf(nb * HEADS * N)
    delta_b, delta = flat_buf(nb * HEADS * N)
    guarded = dict(qkv=(qkv_b, rows), d_o=(do_b, rows), o=(o_b, rows), dqkv=(dqkv_b, rows), lse=(lse_b, nb * HEADS * N), delta=(delta_b, nb * HEADS * N))
    cos = dsin = dfreqs = None
    freqs = inp["freqs"].cuda()
    if HW:
        row = HEADS * half
        cos_b = torch.cat([torch.full((HW * row,), float("nan")), guard_vals((guard * row,), torch.float32, unit=True)]).cuda()
        dsin_b = torch.cat([torch.full((2 * HW * row,), float("nan")), guard_vals((guard * row,), torch.float32, unit=True)]).cuda()
        cos, dsin = cos_b[:HW * row].view(HW, HEADS, half), dsin_b[:2 * HW * row].view(2, HW, HEADS, half)
        ops.rope_cos_table(freqs, H, W, out=cos, dsin=dsin)
        dfreqs = torch.zeros(2, HEADS, half, device="cuda")
        guarded.update(cos=(cos_b, HW * row), dsin=(dsin_b, 2 * HW * row))
    mask, kw = None, {}
    if inp["mask"] is not None:
        Np = inp["mask"].shape[-1]
        extra = (torch.rand(guard, Np, generator=gen) >= RATE).to(torch.uint8)
        mask_b = torch.cat([inp["mask"].reshape(-1, Np), extra ^ 1 if flip_mask_guard else extra]).cuda()
        mask = mask_b[:nb * HEADS * N].view(nb, HEADS, N, Np)
        kw = dict(drop_mask=mask, drop_rate=RATE)
        guarded.update(mask=(mask_b, nb * HEADS * N))
    before = {k: bits(t[n:]).clone() for k, (t, n) in guarded.items()}
    ops.attn_fwd(qkv, cos, o, lse, nb, N, E, HEADS, **kw)
    fam_f = L.lib().lnx_last_attn_kernel()
    ops.attn_bwd(qkv, cos, o, lse, d_o, dqkv, delta, nb, N, E, HEADS, dsin=dsin, dfreqs=dfreqs, **kw)
    fam_b = L.lib().lnx_last_attn_kernel()
    torch.cuda.synchronize()
    assert fam_f == fam_b, (fam_f, fam_b)
    written = [k for k, (t, n) in guarded.items() if not torch.equal(bits(t[n:]), before[k])]
    assert not written, f"rows past the end were written: {written}"
    out = dict(o=o.cpu(), lse=lse.cpu(), dqkv=dqkv.cpu(), delta=delta.cpu(), dfreqs=None if dfreqs is None else dfreqs.cpu(), family=fam_f)
    for k in ("o", "lse", "dqkv", "delta"):
        assert not torch.isnan(out[k]).any(), f"{k}: {int(torch.isnan(out[k]).any(-1).sum())} rows hold a NaN (not written)"
    return out


def check_against_fp64(dtype, hd, case, drop, table):
    N, H, W, E = case
    inp = make_inputs(dtype, hd, case, drop)
    got = launch(inp)
    assert got["family"] == family_of(table, dtype, hd, N), (got["family"], DTN[dtype], hd, N)
    qr = inp["qkv"].double().requires_grad_(True)
    fr = inp["freqs"].double().requires_grad_(True)
    keep = None if not drop else inp["mask"][..., :N].double() / (1.0 - RATE)
    ref = attn_ref(qr, fr, B, N, E, HEADS, hd, H, W, keep)
    ref.backward(inp["d_o"].double())
    tol = 3e-5 if dtype == L.F32 else 2e-2
    tolb = 1e-4 if dtype == L.F32 else 4e-2
    err = lambda a, b: float((a.double() - b).abs().max())  # noqa: E731
    print(f"{DTN[dtype]} hd{hd} {case_id(case)} drop={int(drop)} family={got['family']}: max err o {err(got['o'], ref.detach()):.3e}"
          f" dqkv {err(got['dqkv'], qr.grad):.3e}" + (f" dfreqs {err(got['dfreqs'], fr.grad):.3e} of {float(fr.grad.abs().max()):.3e}" if H * W else ""))
    torch.testing.assert_close(got["o"].double(), ref.detach(), rtol=tol, atol=tol)
    torch.testing.assert_close(got["dqkv"].double(), qr.grad, rtol=tolb, atol=tolb)
    if H * W:
        scale = fr.grad.abs().max().item()
        torch.testing.assert_close(got["dfreqs"].double(), fr.grad, rtol=tolb, atol=tolb * max(scale, 1.0))


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=DTN.get)
def test_sweep_against_fp64(dtype, hd, case, monkeypatch):
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    check_against_fp64(dtype, hd, case, False, FAMILY)


@pytest.mark.parametrize("case", THIN_CASES, ids=case_id)
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=DTN.get)
def test_sweep_with_dropout_mask(dtype, hd, case, monkeypatch):
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    check_against_fp64(dtype, hd, case, True, FAMILY_DROP)


@pytest.mark.parametrize("case", THIN_CASES, ids=case_id)
def test_sweep_tiled_switch(case, monkeypatch):
    """LNX_ATTN_TILED=1 (read per call): bf16 head_dim 64 on the tiled kernels at the lengths the resident ones take by default --
    the only way to attn_fwd_kernel<bf16, 4, false, 64> and its two backward partners"""
    monkeypatch.setenv("LNX_ATTN_TILED", "1")
    check_against_fp64(L.BF16, 64, case, False, FAMILY_TILED_SWITCH)


DECISIVE_NS = [33, 65, 97, 129, 193, 257, 260, 321, 513, 1028]  # a last tile with 1, 4 or 33 live rows, in every family


@pytest.mark.parametrize("N", DECISIVE_NS)
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=DTN.get)
def test_forward_where_a_padding_key_would_decide(dtype, hd, N, monkeypatch):
    """The forward on inputs that turn a padding key into the whole answer.  The kernels make their own padding (zeroed or clamped rows
    of LDS images), which no guard row or neighbour can poison, and the table in the module docstring says the bf16 tolerance does
    not see a zero-score key among random ones.  Here every real score is the same -4 head_dim^0.5 (q = 2, k = -2 in every column,
    all bf16-exact, no image tokens so no cos factor): the output is the plain mean of v, a key of score 0 let into the softmax
    would outweigh all N real keys by e^22 or more and pull o to 0, and the last row of v is 64 times larger than the others, so
    that a clamped copy of key N - 1 counted twice moves o by about 64 / N of a standard deviation.  Same reference and forward
    tolerance as the sweep."""
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    C_ = HEADS * hd
    inp = make_inputs(dtype, hd, (N, 0, 0, N), False)
    qkv = inp["qkv"].view(B, N, 3, C_)
    qkv[:, :, 0], qkv[:, :, 1] = 2.0, -2.0
    qkv[:, N - 1, 2] *= 64.0
    got = launch(inp)
    assert got["family"] == family_of(FAMILY, dtype, hd, N), (got["family"], DTN[dtype], hd, N)
    ref = attn_ref(inp["qkv"].double(), inp["freqs"].double(), B, N, N, HEADS, hd, 0, 0)
    tol = 3e-5 if dtype == L.F32 else 2e-2
    print(f"{DTN[dtype]} hd{hd} N{N} decisive family={got['family']}: max err o {float((got['o'].double() - ref).abs().max()):.3e} of {float(ref.abs().max()):.3e}")
    torch.testing.assert_close(got["o"].double(), ref, rtol=tol, atol=tol)


NW4_SET = os.environ.get("LNX_ATTN_NW") == "4"


@pytest.mark.skipif(not NW4_SET, reason="LNX_ATTN_NW is latched per process: run by test_forced_four_wave_tiles_in_a_child_process")
@pytest.mark.parametrize("case", THIN_CASES, ids=case_id)
@pytest.mark.parametrize("hd", [64, 128])
def test_nw4_sweep(hd, case, monkeypatch):
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    check_against_fp64(L.BF16, hd, case, False, FAMILY_NW4)


@pytest.mark.skipif(NW4_SET, reason="this process is the child")
def test_forced_four_wave_tiles_in_a_child_process():
    """LNX_ATTN_NW=4 (64-row tiles at every length) for bf16 head_dim 64 and 128: one fresh process runs the nw4 cases."""
    want = 2 * len(THIN_CASES)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", __file__, "-q", "-k", "nw4", "-p", "no:cacheprovider"], cwd=REPO,
                           env={**os.environ, "LNX_ATTN_NW": "4"}, timeout=900, capture_output=True, text=True)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the LNX_ATTN_NW=4 child hung; nothing more is started on the GPU\n{e.stdout}", returncode=1)
    tail = "\n".join(r.stdout.strip().splitlines()[-30:])
    if r.returncode < 0 or r.returncode in (134, 139):
        pytest.exit(f"the LNX_ATTN_NW=4 child died (status {r.returncode}); nothing more is started on the GPU\n{tail}\n{r.stderr[-2000:]}", returncode=1)
    assert r.returncode == 0, tail
    m = re.search(r"(\d+) passed", r.stdout.strip().splitlines()[-1])
    assert m and int(m.group(1)) == want and "failed" not in r.stdout.strip().splitlines()[-1], tail


EXACT_CASES = [(c, False) for c in CASES] + [(c, True) for c in THIN_CASES]


@pytest.mark.parametrize("case,drop", EXACT_CASES, ids=lambda v: case_id(v) if isinstance(v, tuple) else ("drop" if v else "plain"))
@pytest.mark.parametrize("hd", [32, 64, 128])
@pytest.mark.parametrize("dtype", [L.F32, L.BF16], ids=DTN.get)
def test_nothing_outside_the_sequence_matters(dtype, hd, case, drop, monkeypatch):
    """Guard bands stay untouched (asserted inside launch); sample 0's o, lse, dqkv, delta are bit-identical whether sample 1 and the
    guards hold ordinary values or |x| = 1e3, and whatever the dropout mask holds in its padding columns and guard rows; dfreqs (a
    sum over samples with LDS float atomics) with one sample, the guards alone changing, within the two-runs-of-one-call bound of
    test_attention_bwd_postponed_freqs_folds_in_one_launch."""
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    N, H, W, E = case
    table = FAMILY_DROP if drop else FAMILY
    inp = make_inputs(dtype, hd, case, drop)
    first = lambda r: dict(o=r["o"][:N], lse=r["lse"][0], dqkv=r["dqkv"][:N], delta=r["delta"][0])  # noqa: E731
    a = launch(inp, guard=G)
    assert a["family"] == family_of(table, dtype, hd, N), (a["family"], DTN[dtype], hd, N)
    a2 = launch(inp, guard=G)
    unstable = [k for k in ("o", "lse", "dqkv", "delta") if not same_bits(a[k], a2[k])]
    assert not unstable, f"control: {unstable} differ between two runs of the same call"
    b = launch(with_big_second_sample(inp), guard=G, big=True)
    assert not same_bits(a["o"][N:], b["o"][N:]), "the second sample was not replaced: this comparison would prove nothing"
    leaked = [k for k, v in first(a).items() if not same_bits(v, first(b)[k])]
    assert not leaked, f"sample 0's {leaked} depend on what lies behind the sequence (sample 1 / guard rows)"
    if drop:
        c = launch(with_flipped_mask_padding(inp), guard=G, flip_mask_guard=True)
        leaked = [k for k in ("o", "lse", "dqkv", "delta") if not same_bits(a[k], c[k])]
        assert not leaked, f"{leaked} depend on the dropout mask's padding columns / guard rows"
    if H * W:
        one = make_inputs(dtype, hd, case, drop, batch=1)
        fa = launch(one, guard=G)["dfreqs"]
        fb = launch(one, guard=G, big=True)["dfreqs"]
        torch.testing.assert_close(fb, fa, rtol=1e-5, atol=1e-5 * float(fa.abs().max()))
        if drop:
            fc = launch(with_flipped_mask_padding(one), guard=G, flip_mask_guard=True)["dfreqs"]
            torch.testing.assert_close(fc, fa, rtol=1e-5, atol=1e-5 * float(fa.abs().max()))
