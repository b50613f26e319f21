"""Deterministic mode, host side (no GPU): the switch, its environment variable, the tile schedule that follows it and the scratch
queries of its fixed-order routes."""
import os
import re
import subprocess
import sys

import pytest

import linnaeus_amd
from linnaeus_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["lnx_attn_bwd_sized", "lnx_set_deterministic", "lnx_get_deterministic", "lnx_tile_sched_static", "lnx_dwconv7_wgrad_ws_floats", "lnx_layerscale_bwd_ws",
               "lnx_layerscale_bwd_ws_floats"]


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    L.lib().lnx_set_deterministic(0)


def test_exports_are_in_the_header_and_the_binding():
    header = open(os.path.join(REPO, "include", "lnx.h")).read()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/lnx.h"
        assert name in L.EXPORTS and hasattr(L.lib(), name), name
    # the tail fields of the argument structs are mirrored (tests/test_abi.py compares the layouts)
    assert [f[0] for f in L.DwconvWgradArgs._fields_][-2:] == ["ws", "ws_floats"]
    assert L.SoftCEArgs._fields_[-1][0] == "sum_ws"


def test_switch_round_trips_and_returns_the_previous_value():
    lib = L.lib()
    lib.lnx_set_deterministic(0)
    assert lib.lnx_get_deterministic() == 0 and not linnaeus_amd.is_deterministic()
    assert lib.lnx_set_deterministic(1) == 0
    assert lib.lnx_get_deterministic() == 1 and linnaeus_amd.is_deterministic()
    assert lib.lnx_set_deterministic(7) == 1 and lib.lnx_get_deterministic() == 1  # any non-zero value switches it on
    assert lib.lnx_set_deterministic(0) == 1 and lib.lnx_get_deterministic() == 0
    assert linnaeus_amd.set_deterministic(True) is False and linnaeus_amd.set_deterministic(False) is True


@pytest.mark.parametrize("value,want", [("1", "1 1"), ("0", "0 0"), (None, "0 0")])
def test_environment_variable_sets_the_initial_value(value, want):
    env = {k: v for k, v in os.environ.items() if k not in ("LNX_DETERMINISTIC", "LNX_TILE_SCHED")}
    if value is not None:
        env["LNX_DETERMINISTIC"] = value
    code = "from linnaeus_amd import _lib as L; print(L.lib().lnx_get_deterministic(), L.lib().lnx_tile_sched_static())"
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == want


def test_tile_schedule_follows_the_switch(monkeypatch):
    lib = L.lib()
    monkeypatch.delenv("LNX_TILE_SCHED", raising=False)
    lib.lnx_set_deterministic(0)
    assert lib.lnx_tile_sched_static() == 0  # the persistent kernels draw their tiles
    lib.lnx_set_deterministic(1)
    assert lib.lnx_tile_sched_static() == 1  # ... and stride over them in the mode
    lib.lnx_set_deterministic(0)
    assert lib.lnx_tile_sched_static() == 0


def test_scratch_queries():
    lib = L.lib()
    dw, ls = lib.lnx_dwconv7_wgrad_ws_floats, lib.lnx_layerscale_bwd_ws_floats
    # refused shapes: 0
    assert dw(2, 28, 28, 48, L.F32, L.F32) == 0      # C is no multiple of 32
    assert dw(0, 28, 28, 32, L.F32, L.F32) == 0
    assert dw(2, 28, 28, 32, 5, L.F32) == 0          # no such dtype
    assert ls(100, 6) == 0 and ls(0, 96) == 0 and ls(100, 2048) == 0
    # walkers x (49 C + C): whole rows of the partial-sum table, at least one, never more walkers than tiles
    for xd, dyd in ((L.F32, L.F32), (L.F32, L.BF16), (L.BF16, L.BF16)):
        for C_ in (32, 96):
            n = dw(2, 28, 28, C_, xd, dyd)
            assert n > 0 and n % (50 * C_) == 0
            assert dw(1, 7, 7, C_, xd, dyd) == 50 * C_   # one tile: one walker
    assert ls(3001, 96) == 38 * 96 and ls(10 ** 7, 96) == 2048 * 96  # 10 rows a pass, 8 passes a workgroup; 2048 workgroups at most
    # the attention backward's workspace grows by its per-wave slots while the mode is on
    att = lib.lnx_attn_bwd_ws_floats_hd
    off = att(2, 260, 2, 64)
    lib.lnx_set_deterministic(1)
    assert att(2, 260, 2, 64) == 17 * off and att(2, 260, 2, 48) == 0
    lib.lnx_set_deterministic(0)
    assert att(2, 260, 2, 64) == off == 2 * 2 * 5 * 64
    # the conv-MLP backward leaves a [2C] LayerNorm row and a [C] dgamma row per WAVE (8 a workgroup) instead of [2C] per workgroup
    cm = lib.lnx_convmlp_bwd_ws_floats
    for C_, M in ((32, 3000), (96, 3000), (192, 3000)):
        small = cm(C_, M)
        lib.lnx_set_deterministic(1)
        assert small > 0 and cm(C_, M) == 12 * small and cm(48, M) == 0 and cm(C_, 0) == 0
        lib.lnx_set_deterministic(0)
    assert "lnx_attn_bwd_sized" in L.EXPORTS
