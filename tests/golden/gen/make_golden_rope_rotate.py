#!/usr/bin/env python3
"""Generate tests/golden/rope_rotate_ops.npz and tiny_rot_hd64.npz / tiny_rot_hd32.npz / tiny_rot_hd128.npz: what the reference's
own RoPE helpers compute when they are handed the COMPLEX table (the true pair rotation, MODEL.ROPE_STAGES.ROPE_ROTATE here)
instead of its real part (what RoPE2DAttention._get_current_freqs_cis leaves after its cast to float32, finding F1).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_rope_rotate.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/ and runs on CPU.  Run by hand, never by a
test.  Writes numbers and names only.

rope_rotate_ops.npz, per case i of OPS (heads, D, H, W, E; B = 1):
  freqs_i [2, heads, D/2], q_i / k_i [B, heads, H W, D] (seeded, fp32)                                  inputs
  cis_re_i / cis_im_i [H W, heads, D/2]     the complex64 table of the reference's compute_mixed_cis(freqs, t_x, t_y)
  q_out_i / k_out_i                         the reference's apply_rotary_emb(q, k, that table)
  wq_i / wk_i, gq_i / gk_i / gf_i           seeded weights of the fixed scalar L = sum(wq q_out) + sum(wk k_out), and its fp64 autograd
                                            gradients with respect to q, k and freqs.  The reference's helpers cast to float32
                                            inside, so the fp64 chain is written here with the same torch complex operations
                                            (polar, view_as_complex, complex product) on float64 inputs.

tiny_rot_hd*.npz: tiny_a of tests/cases.py at 64 px, batch 2 (head_dim 64), and the head splits of make_golden_headdim.py
(head_dim 32 / 128), built by the reference's build_model, with RoPE2DAttention._get_current_freqs_cis replaced at run time by a
function that returns compute_mixed_cis(...) without the cast.  Records of make_golden.run_case (x, meta, feats, logits, loss,
grad_names / grad_norms / grad_sums / gradslice_*) plus every attn.freqs gradient in full (gradfull_*).  run_case itself is not
reused: it cross-checks the cos-only oracle on the way.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "models", "blocks", "rope_2d_mhsa.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(HERE, "_stubs"), REPO, REF, HERE]
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import mformer_oracle as O  # noqa: E402
from tests.cases import CASES, SEED  # noqa: E402

import make_golden as MG  # noqa: E402  (after tests.cases: it puts the checkout, whose tests/ package differs, first on the path)

from linnaeus.models.blocks import rope_2d_mhsa as R  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
IMG, BATCH = 64, 2
HEADS = {"tiny_rot_hd64": (2, 4), "tiny_rot_hd32": (4, 8), "tiny_rot_hd128": (1, 2)}
OPS = [(2, 32, 3, 5, 3), (3, 64, 4, 4, 1), (1, 128, 2, 7, 4), (2, 64, 3, 6, 4)]
OPS_BATCH = 1


def uncast_freqs_cis(self, H, W, device):
    """_get_current_freqs_cis (rope_2d_mhsa.py:397-408) without its last line's cast: the complex table itself"""
    t_x, t_y = R.init_t_xy(W, H, device=device)
    return R.compute_mixed_cis(self.freqs.to(device), t_x, t_y)


def op_records():
    rec = {"n_cases": np.array(len(OPS)), "cases": np.array(OPS)}
    for i, (heads, D, H, W, E) in enumerate(OPS):
        gen = torch.Generator().manual_seed(SEED + 100 + i)
        freqs = O.seeded_fill(f"rot.ops.{i}.freqs", (2, heads, D // 2), SEED)
        q = torch.randn(OPS_BATCH, heads, H * W, D, generator=gen)
        k = torch.randn(OPS_BATCH, heads, H * W, D, generator=gen)
        wq = torch.randn(OPS_BATCH, heads, H * W, D, generator=gen)
        wk = torch.randn(OPS_BATCH, heads, H * W, D, generator=gen)
        t_x, t_y = R.init_t_xy(W, H)
        cis = R.compute_mixed_cis(freqs, t_x, t_y)
        assert cis.dtype == torch.complex64 and cis.shape == (H * W, heads, D // 2)
        q_out, k_out = R.apply_rotary_emb(q, k, cis)
        # fp64 autograd through the same complex operations
        fd, qd, kd = (t.double().requires_grad_(True) for t in (freqs, q, k))
        ang = torch.einsum("n,hd->nhd", t_x.double(), fd[0]) + torch.einsum("n,hd->nhd", t_y.double(), fd[1])
        cis64 = torch.polar(torch.ones_like(ang), ang).permute(1, 0, 2).unsqueeze(0)
        rot = lambda t: torch.view_as_real(torch.view_as_complex(t.reshape(OPS_BATCH, heads, H * W, D // 2, 2)) * cis64).flatten(-2)  # noqa: E731
        qo64, ko64 = rot(qd), rot(kd)
        assert (qo64.detach() - q_out.double()).abs().max().item() < 1e-5
        ((qo64 * wq.double()).sum() + (ko64 * wk.double()).sum()).backward()
        for nm, t in (("freqs", freqs), ("q", q), ("k", k), ("cis_re", cis.real), ("cis_im", cis.imag), ("q_out", q_out), ("k_out", k_out),
                      ("wq", wq), ("wk", wk), ("gq", qd.grad), ("gk", kd.grad), ("gf", fd.grad)):
            rec[f"{nm}_{i}"] = t.detach().contiguous().numpy()
    np.savez_compressed(os.path.join(OUT, "rope_rotate_ops.npz"), **rec)
    print(f"[rope_rotate_ops] {len(OPS)} cases")


def model_case(name):
    a = CASES["tiny_a"]
    spec = O.Spec(conv_dims=a.conv_dims, conv_depths=a.conv_depths, rope_depths=a.rope_depths, rope_heads=HEADS[name], heads=a.heads)
    cfg = MG.apply_spec(MG.base_cfg(IMG), spec, "Linear")
    model = MG.build_model(cfg, num_classes={t: c for t, c in spec.heads})
    ref_sd = MG.load_seeded(model, SEED)
    assert list(O.param_shapes(spec).keys()) == list(ref_sd.keys())
    x, meta = O.seeded_inputs(spec, BATCH, IMG, SEED + 1)
    rec = {"x": x.numpy(), "meta": meta.numpy(), "img": np.array(IMG), "batch": np.array(BATCH)}
    model.eval()
    for p_ in model.parameters():
        p_.requires_grad_(True)
    rec["feats"] = model.forward_features(x, meta).detach().numpy()
    out = model(x, meta)
    for t, lg in out.items():
        rec["logits_" + t] = lg.detach().numpy()
    loss = O.probe_loss(out)
    rec["loss"] = np.array(loss.item())
    model.zero_grad()
    loss.backward()
    grads = {k: p_.grad for k, p_ in model.named_parameters()}
    names = sorted(grads)
    rec["grad_names"] = np.array(names)
    rec["grad_norms"] = np.array([grads[k].double().norm().item() for k in names])
    rec["grad_sums"] = np.array([grads[k].double().sum().item() for k in names])
    for k in names:
        rec["gradslice_" + k] = MG.first_slice(grads[k], 8)
        if k.endswith("attn.freqs"):
            rec["gradfull_" + k] = grads[k].detach().numpy()
    # the rotation must differ from the cos-only oracle (otherwise the patch did not take)
    with torch.no_grad():
        ofe = O.forward_features({k: v for k, v in ref_sd.items()}, spec, x, meta, None)
    diff = (ofe - torch.from_numpy(rec["feats"])).abs().max().item()
    assert diff > 1e-3, diff
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), **rec)
    print(f"[{name}] loss {loss.item():.6f}, max|feats - cos-only oracle| = {diff:.3e}")


def main():
    torch.set_num_threads(8)
    op_records()
    R.RoPE2DAttention._get_current_freqs_cis = uncast_freqs_cis
    for name in HEADS:
        model_case(name)


if __name__ == "__main__":
    main()
