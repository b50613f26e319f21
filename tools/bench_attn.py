"""Attention forward / backward at the mFormerV1_sm stage-3 / stage-4 shapes (B = 256) and the lg @384 stage-3 shape (B = 64, N = 580,
the tiled kernels); run it under `rocprofv3 --kernel-trace --stats` for per-kernel times (the backward is one kernel or two + the
freqs-gradient reduce).  Where the resident backward runs as one kernel (`lnx_last_attn_bwd_launches() == 1`), the dq / dk-dv pair
is timed beside it in the same process (`bwd/pair`: LNX_ATTN_BWD_SPLIT set for those calls, the rounds of the two interleaved).

    python tools/bench_attn.py [--rope-mode cos|rotate|both] [--rounds R]

--rope-mode: the cos-only scaling (default, what the reference runs), the pair rotation (MODEL.ROPE_STAGES.ROPE_ROTATE), or both
side by side.  Every figure is the median of R rounds of 20 calls, with the spread (max - min) / median of the rounds beside it:
two figures closer than the spread are the same figure.  With LNX_LIB_PATH / LNX_LIB_OLDER=1 (linnaeus_amd/_lib.py) the cos mode
runs against another build of the library."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linnaeus_amd import _lib as L
from linnaeus_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rope-mode", choices=("cos", "rotate", "both"), default="cos")
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
modes = ("cos", "rotate") if args.rope_mode == "both" else (args.rope_mode,)

for B, H, W, E, heads in ((256, 14, 14, 3, 6), (256, 7, 7, 3, 12), (64, 24, 24, 4, 12)):
    N = H * W + E
    Cc = heads * 64
    qkv = torch.randn(B * N, 3 * Cc, device="cuda").bfloat16()
    freqs = torch.randn(2, heads, 32, device="cuda")
    dsin = torch.empty(2, H * W, heads, 32, device="cuda")
    cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
    sin = ops.rope_cossin_table(freqs, H, W)[1] if "rotate" in modes else None
    o = torch.empty(B * N, Cc, device="cuda", dtype=torch.bfloat16)
    lse = torch.empty(B * heads * N, device="cuda")
    do = torch.randn_like(o)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    dfreqs = torch.zeros(2, heads, 32, device="cuda")

    for mode in modes:
        if mode == "cos":
            def fwd():
                ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads)

            def bwd():
                ops.attn_bwd(qkv, cos, o, lse, do, dqkv, delta, B, N, E, heads, dsin=dsin, dfreqs=dfreqs)
        else:
            def fwd():
                ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads, sin_tab=sin)

            def bwd():
                ops.attn_bwd(qkv, cos, o, lse, do, dqkv, delta, B, N, E, heads, dfreqs=dfreqs, sin_tab=sin, grid_w=W)

        def rounds(fns):
            """median and spread of R rounds of 20 calls of every fn, the rounds of the fns taking turns"""
            for fn in fns:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            ts = [[] for _ in fns]
            for _ in range(args.rounds):
                for fn, t in zip(fns, ts):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    t.append(e0.elapsed_time(e1) / 20 * 1e-3)
            return [(statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for t in ts]

        def bwd_pair():
            os.environ["LNX_ATTN_BWD_SPLIT"] = "1"  # read per call
            try:
                bwd()
            finally:
                del os.environ["LNX_ATTN_BWD_SPLIT"]

        def show(name, t, spread, fl):
            print(f"N={N} heads={heads} {mode:6s} {name}: {t * 1e6:7.1f} us  spread {100 * spread:4.1f} %  "
                  f"{fl * B * heads * N * N * 64 / t / 1e12:6.1f} TFLOP/s", flush=True)

        (t, sp), = rounds([fwd])
        show("fwd", t, sp, 4.0)
        bwd()
        one_kernel = hasattr(L.lib(), "lnx_last_attn_bwd_launches") and L.lib().lnx_last_attn_bwd_launches() == 1
        if one_kernel:
            (t, sp), (t2, sp2) = rounds([bwd, bwd_pair])
            show("bwd", t, sp, 14.0)
            show("bwd/pair", t2, sp2, 14.0)
            print(f"    one kernel against the pair: {(t2 - t) * 1e6:+.1f} us ({100 * (t2 - t) / t2:+.1f} %); larger spread {100 * max(sp, sp2):.1f} %", flush=True)
        else:
            (t, sp), = rounds([bwd])
            show("bwd", t, sp, 14.0)
