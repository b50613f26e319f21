"""Diagnostic: cycle shares of wave 0 of one workgroup of the resident attention backward at the sm stage-3 shape (needs a library built
with -DATT_STAMP, tools/build_stamp.sh, via LNX_LIB_PATH): the one-kernel backward by default, the dk/dv kernel of the pair with
LNX_ATTN_BWD_SPLIT=1.  (Wave 0 of the one-kernel backward has no dk / dv tile at N = 199 -- the tile rotation, csrc/attention.hip -- so
its phase A columns read 0.)"""
import ctypes as C, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from linnaeus_amd import ops, _lib as L

B, H, W, E, heads = 256, 14, 14, 3, 6
N = H * W + E
Cc = heads * 64
qkv = torch.randn(B * N, 3 * Cc, device="cuda").bfloat16()
freqs = torch.randn(2, heads, 32, device="cuda")
dsin = torch.empty(2, H * W, heads, 32, device="cuda")
cos = ops.rope_cos_table(freqs, H, W, dsin=dsin)
o = torch.empty(B * N, Cc, device="cuda", dtype=torch.bfloat16)
lse = torch.empty(B * heads * N, device="cuda")
ops.attn_fwd(qkv, cos, o, lse, B, N, E, heads)
do = torch.randn_like(o)
dqkv = torch.empty_like(qkv)
dfreqs = torch.zeros(2, heads, 32, device="cuda")
delta = torch.empty_like(lse)
for _ in range(3):
    ops.attn_bwd(qkv, cos, o, lse, do, dqkv, delta, B, N, E, heads, dsin=dsin, dfreqs=dfreqs)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10):
    ops.attn_bwd(qkv, cos, o, lse, do, dqkv, delta, B, N, E, heads, dsin=dsin, dfreqs=dfreqs)
e1.record(); torch.cuda.synchronize()
one = L.lib().lnx_last_attn_bwd_launches() == 1
print("attn_bwd (%s) us:" % ("one kernel" if one else "dq + dkv"), e0.elapsed_time(e1) * 100)
out = (C.c_ulonglong * 8)()
L.lib().lnx_dbg_attn_stamps(out)
names = (["stage", "barrier", "fragments+delta", "barrier", "B key loop", "B epilogue", "A query loop", "A epilogue"] if one
         else ["stage", "stats+barrier", "tile fetch", "q loop", "epilogue"])
tot = sum(out[:len(names)])
print("wave 0: total clk", tot, " | ".join(f"{n} {out[i]} ({out[i] / tot * 100:.1f}%)" for i, n in enumerate(names)))
