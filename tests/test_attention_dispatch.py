"""lnx_attn_dispatch (no GPU): the kernel family lnx_attn_fwd / lnx_attn_bwd take per (dtype, head_dim, N, dropout mask), against
the table of include/lnx.h written out as literal values.  The entry points launch by the same function, and the GPU sweep
(test_gpu_attention_boundaries.py) asserts lnx_last_attn_kernel() against the same literals after real launches.  The in-process
tables are those of a process started without LNX_ATTN_NW (an A/B switch, latched on first use)."""
import json
import os
import subprocess
import sys

from linnaeus_amd import _lib as L

R4, R8, T4, T8 = L.ATTN_KERNEL_RES4, L.ATTN_KERNEL_RES8, L.ATTN_KERNEL_TILED4, L.ATTN_KERNEL_TILED8
NS = [1, 64, 65, 128, 129, 256, 257, 1028]
# (dtype, head_dim, has_drop_mask) -> family at each N of NS
DEFAULT = {
    (L.F32, 32, 0): [T4] * 8, (L.F32, 64, 0): [T4] * 8, (L.F32, 128, 0): [T4] * 8,
    (L.F32, 32, 1): [T4] * 8, (L.F32, 64, 1): [T4] * 8, (L.F32, 128, 1): [T4] * 8,
    (L.BF16, 32, 1): [T4] * 8, (L.BF16, 64, 1): [T4] * 8, (L.BF16, 128, 1): [T4] * 8,
    (L.BF16, 32, 0): [T4] * 8,
    (L.BF16, 64, 0): [R4, R4, R8, R8, R8, R8, T8, T8],
    (L.BF16, 128, 0): [T4, T4, T4, T4, T8, T8, T8, T8],
}
TILED = dict(DEFAULT)
TILED[(L.BF16, 64, 0)] = [T4, T4, T4, T4, T8, T8, T8, T8]
NW4 = dict(DEFAULT)  # LNX_ATTN_NW=4: no 128-row tiles; the resident kernels keep what they take
NW4[(L.BF16, 64, 0)] = [R4, R4, R8, R8, R8, R8, T4, T4]
NW4[(L.BF16, 128, 0)] = [T4] * 8


def table(lib):
    return {k: [lib.lnx_attn_dispatch(k[0], n, k[1], k[2]) for n in NS] for k in DEFAULT}


def test_enum_values_match_the_header():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lnx.h")).read()
    for name, val in (("NONE", 0), ("RES4", R4), ("RES8", R8), ("TILED4", T4), ("TILED8", T8)):
        assert f"LNX_ATTN_KERNEL_{name} = {val}" in src
    assert (R4, R8, T4, T8) == (1, 2, 3, 4)


def test_default_table(monkeypatch):
    monkeypatch.delenv("LNX_ATTN_TILED", raising=False)
    assert table(L.lib()) == DEFAULT
    assert L.lib().lnx_attn_dispatch(L.BF16, 100, 0, 0) == R8  # head_dim 0 = 64


def test_tiled_switch_is_read_per_call(monkeypatch):
    lib = L.lib()
    monkeypatch.setenv("LNX_ATTN_TILED", "1")
    assert table(lib) == TILED
    monkeypatch.delenv("LNX_ATTN_TILED")
    assert table(lib) == DEFAULT


def test_four_wave_switch_in_a_fresh_process():
    """LNX_ATTN_NW is latched on first use, so its table comes from a child process."""
    code = ("import json; from linnaeus_amd import _lib as L; lib = L.lib();"
            f"print(json.dumps([[list(k), [lib.lnx_attn_dispatch(k[0], n, k[1], k[2]) for n in {NS}]] for k in {sorted(DEFAULT)}]))")
    env = {**os.environ, "LNX_ATTN_NW": "4"}
    env.pop("LNX_ATTN_TILED", None)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, check=True, capture_output=True, text=True, timeout=300).stdout
    got = {tuple(k): v for k, v in json.loads(out.strip().splitlines()[-1])}
    assert got == NW4


def test_refused_arguments():
    lib = L.lib()
    for hd in (16, 48, 96, 256, -64):
        assert lib.lnx_attn_dispatch(L.BF16, 100, hd, 0) < 0, hd
        assert lib.lnx_attn_dispatch(L.F32, 100, hd, 1) < 0, hd
    assert lib.lnx_attn_dispatch(L.BF16, 0, 64, 0) < 0 and lib.lnx_attn_dispatch(L.F32, -5, 64, 0) < 0
    assert lib.lnx_attn_dispatch(7, 100, 64, 0) < 0


def test_nothing_launched_yet_reports_no_family():
    """lnx_last_attn_kernel is 0 until the first lnx_attn_fwd / lnx_attn_bwd launch of the process (a fresh one: other tests of this
    process may have launched); a refused call leaves it alone."""
    code = ("import ctypes as C; from linnaeus_amd import _lib as L; lib = L.lib(); a = L.AttnArgs(); a.dtype = L.BF16;"
            "a.B, a.N, a.E, a.heads, a.head_dim = 1, 8, 8, 1, 48; a.qkv = a.o = C.c_void_p(0x1000);"
            "rc = lib.lnx_attn_fwd(C.byref(a), None); lib.lnx_attn_dispatch(L.BF16, 8, 64, 0); print(rc != 0, lib.lnx_last_attn_kernel())")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], cwd=root, check=True, capture_output=True, text=True, timeout=300).stdout
    assert out.strip().splitlines()[-1] == "True 0"
