"""FusedMuon without a GPU: the CPU restatement against the reference's recorded steps, the workspace layout and tile tables of
lnx_muon_layout walked on the host, argument validation of the entry points, and the optimizer's constructor / state_dict."""
import ast
import ctypes as C
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from linnaeus_amd import _lib as L
from tests import muon_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = [dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5),
          dict(lr=0.01, weight_decay=0.0, momentum=0.9, nesterov=False, ns_steps=3)]
FIXTURE_SHAPES = [(48, 192), (192, 48), (40, 100), (32, 8, 2, 2), (16, 1, 7, 7), (96, 1, 7, 7)]
GPU_TEST_SHAPES = FIXTURE_SHAPES + [(64, 64), (33, 33), (136, 264), (264, 136), (384, 96), (96, 384), (1152, 384), (384, 1536), (768, 3072), (2304, 768),
                                    (1, 40), (40, 1), (8, 8)]


def flat(shape):
    return (shape[0], int(np.prod(shape[1:])))


def sm_muon_shapes():
    from linnaeus_amd import arch_config, build_model
    from linnaeus_amd.optim import muon_parameters

    tasks = (("taxa_L10", 1000), ("taxa_L20", 300), ("taxa_L30", 80), ("taxa_L40", 20))
    cfg = arch_config("sm", 224)
    cfg.DATA.TASK_KEYS_H5 = [t for t, _ in tasks]
    cfg.MODEL.CLASSIFICATION.HEADS = {t: {"TYPE": "Linear"} for t, _ in tasks}
    return [tuple(p.shape) for p in muon_parameters(build_model(cfg, num_classes=dict(tasks)))]


def test_muon_ref_reproduces_the_reference_bit_for_bit(golden_dir):
    """tests/golden/muon_fused.npz: three steps of the reference's Muon on six parameters in two groups, one gradient missing"""
    z = np.load(f"{golden_dir}/muon_fused.npz")
    # as the generator ran the reference: with torch's own CPU matmul.  oneDNN's bf16 kernels differ from CPU to CPU (AMX, AVX512-BF16,
    # plain AVX512) and round a few elements of a product differently; the fallback gives the same bits on every machine
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with torch.backends.mkldnn.flags(enabled=False):
            check_against_fixture(z)


def check_against_fixture(z):
    assert [ast.literal_eval(str(s)) for s in z["shapes"]] == FIXTURE_SHAPES
    no_grad = tuple(int(v) for v in z["no_grad"])
    for i, shape in enumerate(FIXTURE_SHAPES):
        group = GROUPS[i % 2]
        p, buf = torch.from_numpy(z[f"p{i}_init"]), None
        assert tuple(p.shape) == shape
        for s in range(3):
            g = None if (s, i) == no_grad else torch.from_numpy(z[f"p{i}_grad{s}"])
            p, buf, _ = R.step(p, g, buf, group)
            assert torch.equal(p, torch.from_numpy(z[f"p{i}_after{s}"])), (i, s)
        assert torch.equal(buf, torch.from_numpy(z[f"p{i}_buf"])), i


def test_muon_ref_exact_switch():
    g = torch.Generator().manual_seed(3)
    p, gr = torch.randn(24, 40, generator=g), torch.randn(24, 40, generator=g)
    q, _, o = R.step(p, gr, None, GROUPS[0])
    qe, _, oe = R.step(p, gr, None, GROUPS[0], exact=True)
    assert qe.dtype == torch.float64 and oe.dtype == torch.float64
    assert 0 < (o.double() - oe).abs().max() < 0.1
    torch.testing.assert_close(R.recover_update(p, q, GROUPS[0]).double(), oe, atol=0.1, rtol=0)


def check_layout(shapes):
    from linnaeus_amd.optim import muon_layout

    T = L.MUON_TILE
    mats, tiles, info = muon_layout(shapes)
    regions = []
    blocks = 0
    for i, (rows, cols) in enumerate(shapes):
        m = mats[i]
        assert (m.rows, m.cols) == (rows, cols)
        assert m.mp % T == 0 and m.np % T == 0 and min(rows, cols) <= m.mp < min(rows, cols) + T and max(rows, cols) <= m.np < max(rows, cols) + T
        xb, ab = 2 * m.mp * m.np, 2 * m.mp * m.mp
        for off, size in ((m.x_off, xb), (m.xt_off[0], xb), (m.xt_off[1], xb), (m.a_off, ab), (m.b_off, ab)):
            assert off % 256 == 0 and 0 <= off and off + size <= info.workspace_bytes
            regions.append((off, off + size))
        assert m.block_start == blocks
        blocks += -(-rows * cols // L.MUON_ELEMS)
    assert info.total_blocks == blocks
    regions.sort()
    for (_, e0), (s1, _) in zip(regions, regions[1:]):
        assert e0 <= s1  # pairwise disjoint
    assert info.workspace_bytes == sum(e - s for s, e in regions)  # and nothing wasted between them
    assert tiles.shape == (sum(info.ntiles), 4)
    base = 0
    for s in range(3):
        table = tiles[base:base + info.ntiles[s]]
        pos = 0
        for i in range(len(shapes)):
            m = mats[i]
            tm, tn = m.mp // T, (m.np // T if s == 2 else m.mp // T)
            assert (m.tile_start[s], m.tile_count[s]) == (pos, tm * tn)
            mine = table[pos:pos + tm * tn]
            assert (mine[:, 0] == i).all()
            # every output tile exactly once
            assert sorted(map(tuple, mine[:, 1:3].tolist())) == [(r, c) for r in range(tm) for c in range(tn)]
            # operand extents of a tile: T rows of P at tile row tr and T rows of Q at tile column tc, each K long with leading dimension K
            # (stage 0: P = Q = X, K = np; stage 1: P = Q = A, K = mp; stage 2: P = B, Q = X^T, K = mp), inside their regions
            k = m.np if s == 0 else m.mp
            p_bytes = (2 * m.mp * m.np, 2 * m.mp * m.mp, 2 * m.mp * m.mp)[s]
            q_bytes = (2 * m.mp * m.np, 2 * m.mp * m.mp, 2 * m.mp * m.np)[s]
            assert ((mine[:, 1].astype(np.int64) + 1) * T * k * 2 <= p_bytes).all() and ((mine[:, 2].astype(np.int64) + 1) * T * k * 2 <= q_bytes).all()
            pos += tm * tn
        assert pos == info.ntiles[s]
        base += info.ntiles[s]
    return mats, tiles, info


def test_layout_of_the_fixture_and_gpu_test_shapes():
    check_layout([flat(s) for s in FIXTURE_SHAPES])
    check_layout([flat(s) for s in GPU_TEST_SHAPES])
    check_layout([flat(s) for s in reversed(GPU_TEST_SHAPES)])
    mats, _, _ = check_layout([(136, 264), (264, 136)])
    for i in range(2):  # the multi-tile case of the GPU tests: at least three tiles along m, at least three K steps in every product
        assert mats[i].mp // L.MUON_TILE >= 3 and mats[i].mp // 32 >= 3 and mats[i].np // 32 >= 3


def test_layout_of_the_sm_muon_set():
    shapes = sm_muon_shapes()
    assert len(shapes) == 52  # optimizers/build.py:130-154 on mFormerV1_sm
    _, _, info = check_layout([flat(s) for s in shapes])
    n = sum(int(np.prod(s)) for s in shapes)
    print(f"[muon layout] sm: {n} parameters, workspace {info.workspace_bytes} bytes = {info.workspace_bytes / n:.2f} per parameter")
    assert info.workspace_bytes < 12 * n


def test_ctypes_mirrors_have_the_sizes_the_c_compiler_gives(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in L.MUON_STRUCTS) + "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in L.MUON_STRUCTS.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    assert "lnx_muon_step" in L.EXPORTS and "lnx_muon_layout" in L.EXPORTS and "lnx_muon_launches" in L.EXPORTS


def test_entry_points_validate_on_the_host():
    """nothing here reaches a launch: every call is refused first (the pointers are never dereferenced)"""
    from linnaeus_amd.optim import muon_layout

    lib = L.lib()
    before = lib.lnx_muon_launches()
    info = L.MuonInfo()
    mats = (L.MuonMat * 2)()
    shapes = (C.c_int * 4)(48, 192, 40, 100)
    assert lib.lnx_muon_layout(None, 2, mats, None, 0, C.byref(info)) != 0 and b"lnx_muon_layout" in lib.lnx_last_error()
    assert lib.lnx_muon_layout(shapes, 2, None, None, 0, C.byref(info)) != 0
    assert lib.lnx_muon_layout(shapes, 0, mats, None, 0, C.byref(info)) != 0
    bad = (C.c_int * 4)(48, 0, 40, 100)
    assert lib.lnx_muon_layout(bad, 2, mats, None, 0, C.byref(info)) != 0 and b"shape" in lib.lnx_last_error()
    tiles = np.zeros((4, 4), dtype=np.int32)
    assert lib.lnx_muon_layout(shapes, 2, mats, tiles.ctypes.data, 4, C.byref(info)) != 0 and b"entries" in lib.lnx_last_error()

    mats, _, info = muon_layout([(48, 192), (40, 100)])
    fake = 0x10000

    def args():
        a = L.MuonStepArgs()
        a.n, a.mats, a.mats_dev, a.tiles_dev, a.workspace, a.workspace_bytes, a.partials = 2, C.addressof(mats), fake, fake, fake, info.workspace_bytes, fake
        for i in range(2):
            mats[i].p, mats[i].g, mats[i].buf, mats[i].ns_steps = fake, fake, fake, 5
        return a

    assert lib.lnx_muon_step(None, None) != 0
    for field in ("mats", "mats_dev", "tiles_dev", "workspace", "partials"):
        a = args()
        setattr(a, field, None)
        assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"lnx_muon_step" in lib.lnx_last_error(), field
    a = args()
    a.workspace_bytes -= 1
    assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"workspace bytes" in lib.lnx_last_error()
    a = args()
    a.workspace = fake + 8
    assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"aligned" in lib.lnx_last_error()
    a = args()
    mats[1].ns_steps = -1
    assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"ns_steps" in lib.lnx_last_error()
    for field, delta in (("mp", 32), ("np", 32), ("x_off", 256), ("a_off", -256), ("b_off", 2048), ("block_start", 1)):
        a = args()
        keep = getattr(mats[1], field)
        setattr(mats[1], field, keep + delta)
        assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"does not match the layout" in lib.lnx_last_error(), field
        setattr(mats[1], field, keep)
    a = args()
    mats[1].tile_start[2] += 1
    assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"does not match the layout" in lib.lnx_last_error()
    mats[1].tile_start[2] -= 1
    a = args()
    mats[0].p = None
    assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"parameter pointer" in lib.lnx_last_error()
    a = args()
    mats[0].buf = None
    assert lib.lnx_muon_step(C.byref(a), None) != 0 and b"momentum buffer" in lib.lnx_last_error()
    assert lib.lnx_muon_launches() == before  # refused calls launch nothing


def test_constructor_validation_and_param_groups():
    import linnaeus_amd
    from linnaeus_amd.optim import FusedMuon

    assert linnaeus_amd.FusedMuon is FusedMuon
    w = torch.nn.Parameter(torch.zeros(8, 4))
    for kw in (dict(lr=-1.0), dict(momentum=1.0), dict(momentum=-0.1), dict(weight_decay=-1e-3), dict(ns_steps=-1)):
        with pytest.raises(ValueError):
            FusedMuon([w], **kw)
    for strict in (False, True):  # the reference only refuses other shapes under strict (and then fails in its first step)
        for bad in (torch.zeros(5), torch.zeros(2, 3, 4), torch.zeros(())):
            with pytest.raises(ValueError, match="2D or 4D"):
                FusedMuon([w, torch.nn.Parameter(bad)], strict=strict)
    opt = FusedMuon([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(4, 2, 3, 3))], "lr": 0.01, "nesterov": False, "ns_steps": 3}])
    assert set(opt.param_groups[0]) - {"params"} >= {"lr", "weight_decay", "momentum", "nesterov", "ns_steps"}
    assert [opt.param_groups[0][k] for k in ("lr", "weight_decay", "momentum", "nesterov", "ns_steps")] == [0.02, 0.01, 0.95, True, 5]
    assert [opt.param_groups[1][k] for k in ("lr", "weight_decay", "momentum", "nesterov", "ns_steps")] == [0.01, 0.01, 0.95, False, 3]
    assert opt.step() is None  # no gradients: nothing to do, nothing launched, no state
    assert len(opt.state) == 0
    w.grad = torch.zeros_like(w)
    with pytest.raises(L.LnxError):  # parameters on the CPU
        opt.step()


def test_state_dict_moves_between_fused_muon_and_muon():
    from linnaeus_amd.optim import FusedMuon, Muon

    def make(cls):
        ps = [torch.nn.Parameter(torch.zeros(6, 4)), torch.nn.Parameter(torch.zeros(4, 2, 3, 3))]
        return ps, cls([{"params": ps[:1]}, {"params": ps[1:], "lr": 0.01, "momentum": 0.9, "nesterov": False, "ns_steps": 3}])

    g = torch.Generator().manual_seed(1)
    for src, dst in ((Muon, FusedMuon), (FusedMuon, Muon)):
        ps, a = make(src)
        for p in ps:
            a.state[p]["momentum_buffer"] = torch.randn(p.shape, generator=g)
        sd = a.state_dict()
        qs, b = make(dst)
        b.load_state_dict(sd)
        assert b.state_dict()["param_groups"] == sd["param_groups"]
        for p, q in zip(ps, qs):
            assert set(b.state[q]) == {"momentum_buffer"}
            assert torch.equal(b.state[q]["momentum_buffer"], a.state[p]["momentum_buffer"])
