#!/usr/bin/env python3
"""Generate tests/golden/tiny_hd32.npz, tiny_hd128.npz, tiny_hd_drop.npz and tiny_headdim_params.json from the reference's
own mFormerV1 with attention head sizes other than 64 (RoPE2DAttention takes any head_dim: freqs [2, heads, head_dim/2],
scale head_dim**-0.5, blocks/rope_2d_mhsa.py:76-111).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_golden_headdim.py <linnaeus checkout>

Imports `linnaeus` from the given checkout (read-only) with the stand-ins under _stubs/ and runs on CPU in fp32.  Every case is
tiny_a of tests/cases.py (dims 32/64/128/256, one block per stage, two Linear heads, E = 3 extra tokens at 64 px, batch 2) with
other RoPE head counts:

  tiny_hd32     rope_heads (4, 8): head_dim 32 on both RoPE stages      (make_golden.run_case: logits, loss, gradients)
  tiny_hd128    rope_heads (1, 2): head_dim 128 on both RoPE stages     (make_golden.run_case)
  tiny_hd_drop  rope_heads (4, 2): head_dim 32 then 128, in train mode with DROP_RATE 0.2 / ATTN_DROP_RATE 0.1 and the keep mask
                of every nn.Dropout call (make_golden.run_dropout_case)

tiny_headdim_params.json: the reference's state_dict names and shapes of the tiny_hd32 and tiny_hd128 models, in order.
Writes numbers and names only.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "models", "blocks", "rope_2d_mhsa.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(HERE, "_stubs"), REPO, REF, HERE]
sys.dont_write_bytecode = True

import torch  # noqa: E402

from oracle import mformer_oracle as O  # noqa: E402
from tests.cases import CASES  # noqa: E402

import make_golden as MG  # noqa: E402  (after tests.cases: it puts the checkout, whose tests/ package differs, first on the path)

OUT = os.path.join(REPO, "tests", "golden")
IMG, BATCH = 64, 2
HEADS = {"tiny_hd32": (4, 8), "tiny_hd128": (1, 2), "tiny_hd_drop": (4, 2)}


def spec_of(name):
    a = CASES["tiny_a"]
    return O.Spec(conv_dims=a.conv_dims, conv_depths=a.conv_depths, rope_depths=a.rope_depths, rope_heads=HEADS[name], heads=a.heads)


def main():
    torch.set_num_threads(8)
    params = {}
    for name in ("tiny_hd32", "tiny_hd128"):
        model = MG.run_case(name, spec_of(name), IMG, BATCH)
        params[name] = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    MG.run_dropout_case("tiny_hd_drop", spec_of("tiny_hd_drop"), IMG, BATCH)
    with open(os.path.join(OUT, "tiny_headdim_params.json"), "w") as f:
        json.dump(params, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()
