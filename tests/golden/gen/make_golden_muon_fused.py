#!/usr/bin/env python3
"""Generate tests/golden/muon_fused.npz from the reference's own Muon (linnaeus/optimizers/muon.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_muon_fused.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/, runs three optimizer steps on the
CPU and writes numbers only: the initial parameters, every step's gradients (as given, before the reference overwrites
them with the Nesterov gradient), the parameters after every step and the final momentum buffers.  Inputs are rounded to
bf16-representable fp32 values (exact either way; it keeps the file small).

Parameters p0..p5 of shapes SHAPES; two groups:
  group 0 = p0, p2, p4: lr 0.02, weight_decay 0.01, momentum 0.95, Nesterov, 5 iterations
  group 1 = p1, p3, p5: lr 0.01, weight_decay 0,    momentum 0.9,  no Nesterov, 3 iterations
p3 has no gradient in the second step.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "optimizers", "muon.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
sys.path[:0] = [os.path.join(HERE, "_stubs"), os.path.abspath(sys.argv[1])]
sys.dont_write_bytecode = True

import logging  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

warnings.filterwarnings("ignore")
logging.disable(logging.CRITICAL)

from linnaeus.optimizers.muon import Muon  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "muon_fused.npz")
SEED = 20261019
SHAPES = [(48, 192), (192, 48), (40, 100), (32, 8, 2, 2), (16, 1, 7, 7), (96, 1, 7, 7)]
GROUPS = [dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5),
          dict(lr=0.01, weight_decay=0.0, momentum=0.9, nesterov=False, ns_steps=3)]
MEMBERS = [[0, 2, 4], [1, 3, 5]]
STEPS = 3
NO_GRAD = (1, 3)  # (step, parameter)


def bf16_exact(t):
    return t.to(torch.bfloat16).float()


def main():
    torch.manual_seed(SEED)
    gen = torch.Generator().manual_seed(SEED)
    params = [torch.nn.Parameter(bf16_exact(torch.randn(*s, generator=gen) * 0.1)) for s in SHAPES]
    rec = {"shapes": np.array([str(s) for s in SHAPES]), "no_grad": np.array(NO_GRAD)}
    for i, p in enumerate(params):
        rec[f"p{i}_init"] = p.detach().numpy().copy()
    opt = Muon([dict(params=[params[i] for i in m], **g) for m, g in zip(MEMBERS, GROUPS)])
    for s in range(STEPS):
        for i, p in enumerate(params):
            if (s, i) == NO_GRAD:
                p.grad = None
                continue
            g = bf16_exact(torch.randn(p.shape, generator=gen) * (0.02 + 0.05 * s) * (1.0 + i))
            rec[f"p{i}_grad{s}"] = g.numpy().copy()
            p.grad = g.clone()
        opt.step()
        for i, p in enumerate(params):
            rec[f"p{i}_after{s}"] = p.detach().numpy().copy()
    for i, p in enumerate(params):
        rec[f"p{i}_buf"] = opt.state[p]["momentum_buffer"].numpy().copy()
    np.savez_compressed(OUT, **rec)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    # oneDNN's bf16 matmul kernels differ from CPU to CPU (AMX, AVX512-BF16, plain AVX512) and so do their bits; torch's own
    # fallback gives the same on every machine, and tests/test_muon_fused_host.py runs its restatement the same way
    with torch.backends.mkldnn.flags(enabled=False):
        main()
