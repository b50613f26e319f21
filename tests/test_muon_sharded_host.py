"""ShardedFusedMuon without a GPU: lnx_muon_partition (ownership, segment layout, balance on the sm set), the host refusals of
lnx_muon_partition / lnx_muon_orthogonalize / lnx_muon_apply_packed, the ctypes mirror of lnx_muon_packed, the optimizer's host-side
bookkeeping, and `build_optimizer` under two gloo ranks.  The device path is in tests/test_gpu_muon_sharded.py."""
import ctypes as C
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from linnaeus_amd import _lib as L
from linnaeus_amd.optim import muon_layout, muon_partition

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWELVE = [(48, 192), (192, 48), (40, 100), (64, 64), (33, 33), (16, 49), (96, 49), (32, 32), (136, 264), (264, 136), (8, 8), (1, 40)]
ALIGN = L.MUON_SEG_ALIGN


def cost_of(shape, ns):
    """the rule of include/lnx.h, restated: MFMA FLOPs of the three products on the padded operands"""
    T = L.MUON_TILE
    mp_, np_ = (-(-min(shape) // T) * T), (-(-max(shape) // T) * T)
    return ns * (4 * mp_ * mp_ * np_ + 2 * mp_ ** 3) if ns > 0 else mp_ * np_


def greedy(shapes, ns, world):
    """longest-processing-time greedy, restated: (cost descending, index ascending), least-loaded rank, lowest rank on ties"""
    cost = [cost_of(s, k) for s, k in zip(shapes, ns)]
    load, owner = [0] * world, [None] * len(shapes)
    for i in sorted(range(len(shapes)), key=lambda i: (-cost[i], i)):
        r = min(range(world), key=lambda r: (load[r], r))
        owner[i] = r
        load[r] += cost[i]
    return owner, load


def check_partition(shapes, ns, world):
    owner, off, seg, cost = muon_partition(shapes, ns, world)
    assert muon_partition(shapes, ns, world) == (owner, off, seg, cost)  # a pure function of its inputs
    want_owner, want_load = greedy(shapes, ns, world)
    assert owner == want_owner and cost == want_load
    assert len(owner) == len(shapes) and all(0 <= r < world for r in owner)  # every matrix has one owner
    assert seg % ALIGN == 0
    largest = 0
    for r in range(world):
        mine = [i for i in range(len(shapes)) if owner[i] == r]
        pos = 0
        for i in mine:  # table order, each at the next multiple of 128 elements: disjoint and inside the segment
            assert off[i] == pos and off[i] % ALIGN == 0
            pos += -(-shapes[i][0] * shapes[i][1] // ALIGN) * ALIGN
        assert pos <= seg
        largest = max(largest, pos)
    assert seg == largest
    return owner, off, seg, cost


def test_partition_owners_offsets_and_determinism():
    ns = [5, 3] * 6
    for world in (1, 2, 3, 5, 16):
        owner, off, seg, cost = check_partition(TWELVE, ns, world)
        if world > len(TWELVE):
            assert sorted(set(range(world)) - set(owner)) and cost.count(0) == world - len(TWELVE)  # empty ranks
    owner, off, seg, _ = check_partition(TWELVE, ns, 1)  # one segment in table order
    assert owner == [0] * 12 and off == sorted(off) and seg == sum(-(-r * c // ALIGN) * ALIGN for r, c in TWELVE)
    owner, _, _, cost = check_partition([(64, 64)] * 4, [5] * 4, 2)  # ties: by index, to the lowest rank
    assert owner == [0, 1, 0, 1] and cost[0] == cost[1]
    owner, _, _, cost = check_partition([(64, 64), (40, 100), (64, 64)], [0, 0, 5], 2)  # ns_steps = 0 costs mp np
    assert cost == [cost_of((64, 64), 5), 64 * 64 + 64 * 128] and owner == [1, 1, 0]


def sm_muon_set():
    from linnaeus_amd import build_model
    from linnaeus_amd.optim import muon_parameters
    from tests.cases import CASES, make_config

    spec = CASES["sm"]
    model = build_model(make_config(spec, 224), num_classes={t: c for t, c in spec.heads})
    return model, muon_parameters(model)


@pytest.fixture(scope="module")
def sm_set():
    return sm_muon_set()


def test_balance_on_the_sm_muon_set(sm_set):
    _, params = sm_set
    shapes = [(p.size(0), p.numel() // p.size(0)) for p in params]
    assert len(shapes) == 52
    total = sum(cost_of(s, 5) for s in shapes)
    for world in (2, 3, 4, 8):
        owner, off, seg, cost = check_partition(shapes, [5] * 52, world)
        ratio = max(cost) / (sum(cost) / world)
        print(f"[muon partition] sm, world {world}: max / mean rank cost {ratio:.4f}, seg_elems {seg}, total {total / 1e9:.1f} GFLOP")
        assert sum(cost) == total
        assert ratio <= 1.05, (world, ratio)


def test_partition_report_and_ownership_of_the_optimizer(sm_set):
    from linnaeus_amd.optim import ShardedFusedMuon

    _, params = sm_set
    world = 4
    opts = [ShardedFusedMuon([{"params": params[:30]}, {"params": params[30:], "ns_steps": 3}], rank=r, world_size=world, gather=lambda out, seg: None)
            for r in range(world)]
    reps = [o.partition_report() for o in opts]
    full = int(muon_layout([(p.size(0), p.numel() // p.size(0)) for p in params])[2].workspace_bytes)
    assert all(r["owner"] == reps[0]["owner"] and r["cost"] == reps[0]["cost"] and r["seg_elems"] == reps[0]["seg_elems"] for r in reps)
    assert len(reps[0]["owner"]) == 52 and set(reps[0]["owner"]) == set(range(world))
    assert sum(r["workspace_bytes"] for r in reps) == full  # the layout is additive: every rank holds its share
    assert reps[0]["max_over_mean"] == max(reps[0]["cost"]) / (sum(reps[0]["cost"]) / world)
    for r, o in enumerate(opts):
        assert [o.owns(p) for p in params] == [k == r for k in reps[0]["owner"]]
    # a full state dict (FusedMuon's layout) keeps the owned part only; the local shard loads back
    g = torch.Generator().manual_seed(0)
    from linnaeus_amd.optim import FusedMuon

    ref = FusedMuon([{"params": params[:30]}, {"params": params[30:], "ns_steps": 3}])
    for p in params[:40]:  # (the last 12 never had a gradient)
        ref.state[p]["momentum_buffer"] = torch.randn(p.shape, generator=g)
    sd = ref.state_dict()
    for r, o in enumerate(opts):
        o.load_state_dict(sd)
        assert {id(p) for p in o.state} == {id(p) for k, p in enumerate(params[:40]) if reps[0]["owner"][k] == r}
        for p in o.state:
            assert torch.equal(o.state[p]["momentum_buffer"], ref.state[p]["momentum_buffer"])
        local = o.state_dict()
        assert sorted(local["state"]) == [k for k in range(40) if reps[0]["owner"][k] == r]
        o.load_state_dict(local)
        assert sorted(o.state_dict()["state"]) == sorted(local["state"])
    with pytest.raises(ValueError):
        ShardedFusedMuon(params[:2], rank=2, world_size=2, gather=lambda out, seg: None)
    with pytest.raises(ValueError, match="not initialised"):
        ShardedFusedMuon(params[:2])


def test_full_state_dict_on_the_host_through_the_seam():
    """world of three on the CPU: the state buffers travel through the same seam as the updates"""
    from linnaeus_amd.optim import FusedMuon, ShardedFusedMuon

    world = 3
    g = torch.Generator().manual_seed(1)
    shapes = [(6, 4), (4, 2, 3, 3), (8, 8), (3, 40), (33, 33)]

    def groups(ps):
        return [{"params": ps[:3]}, {"params": ps[3:], "ns_steps": 2}]

    base = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    ref = FusedMuon(groups(base))
    for p in base[:4]:
        ref.state[p]["momentum_buffer"] = torch.randn(p.shape, generator=g)
    opts = []

    def seam(out, seg):
        for r, o in enumerate(opts):  # what an all-gather does: rank r's part of everybody's buffer is rank r's segment
            out.view(world, -1)[r].copy_(o._state_segment())

    for r in range(world):
        opts.append(ShardedFusedMuon(groups([torch.nn.Parameter(torch.zeros(s)) for s in shapes]), rank=r, world_size=world, gather=seam))
        opts[-1].load_state_dict(ref.state_dict())
    want = ref.state_dict()
    for o in opts:
        got = o.full_state_dict()
        assert got["param_groups"] == want["param_groups"] and sorted(got["state"]) == sorted(want["state"]) == [0, 1, 2, 3]
        for k in want["state"]:
            assert set(got["state"][k]) == {"momentum_buffer"} and torch.equal(got["state"][k]["momentum_buffer"], want["state"][k]["momentum_buffer"])
    back = FusedMuon(groups([torch.nn.Parameter(torch.zeros(s)) for s in shapes]))
    back.load_state_dict(opts[1].full_state_dict())  # and it loads where FusedMuon's does
    assert len(back.state) == 4


def test_ctypes_mirror_of_the_packed_table(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lnx.h"\nint main(void) {\n' +
                   "".join(f'    printf("{n} %zu\\n", sizeof({n}));\n' for n in L.MUON_SHARDED_STRUCTS) +
                   "".join(f'    printf("{f} %zu\\n", offsetof(lnx_muon_packed, {f}));\n' for f in ("p", "off", "numel", "decay", "step", "block_start")) +
                   '    printf("align %d\\n", LNX_MUON_SEG_ALIGN);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    for n, cls in L.MUON_SHARDED_STRUCTS.items():
        assert int(got[n]) == C.sizeof(cls), (n, got[n], C.sizeof(cls))
    for f in ("p", "off", "numel", "decay", "step", "block_start"):
        assert int(got[f]) == getattr(L.MuonPacked, f).offset, f
    assert int(got["align"]) == L.MUON_SEG_ALIGN
    for name in ("lnx_muon_partition", "lnx_muon_orthogonalize", "lnx_muon_apply_packed"):
        assert name in L.EXPORTS
    assert L.lib().lnx_version() >= 118


def test_partition_validates_on_the_host():
    lib = L.lib()
    shapes, ns = (C.c_int * 4)(48, 192, 40, 100), (C.c_int * 2)(5, 5)
    owner, off, cost, seg = (C.c_int * 2)(), (C.c_int64 * 2)(), (C.c_int64 * 4)(), C.c_int64()

    def call(shapes=shapes, ns=ns, n=2, world=2, owner=owner, off=off, cost=cost):
        return lib.lnx_muon_partition(shapes, ns, n, world, owner, off, C.byref(seg), cost)

    assert call() == 0
    for kw in (dict(shapes=None), dict(ns=None), dict(owner=None), dict(off=None), dict(cost=None), dict(n=0)):
        assert call(**kw) != 0 and b"lnx_muon_partition" in lib.lnx_last_error(), kw
    for world in (0, -3):
        assert call(world=world) != 0 and b"lnx_muon_partition: world=" in lib.lnx_last_error()
    assert call(ns=(C.c_int * 2)(5, -1)) != 0 and b"ns_steps=-1" in lib.lnx_last_error()
    assert call(shapes=(C.c_int * 4)(48, 0, 40, 100)) != 0 and b"shape" in lib.lnx_last_error()


def test_device_entry_points_validate_on_the_host():
    """nothing here reaches a launch: every call is refused first (the pointers are never dereferenced)"""
    lib = L.lib()
    before = lib.lnx_muon_launches()
    mats, _, info = muon_layout([(48, 192), (40, 100)])
    fake = 0x10000
    off = np.asarray([0, 48 * 192], dtype=np.int64)
    seg_elems = 48 * 192 + 4096

    def args():
        a = L.MuonStepArgs()
        a.n, a.mats, a.mats_dev, a.tiles_dev, a.workspace, a.workspace_bytes, a.partials = 2, C.addressof(mats), fake, fake, fake, info.workspace_bytes, fake
        for i in range(2):
            mats[i].p, mats[i].g, mats[i].buf, mats[i].ns_steps = fake, fake, fake, 5
        return a

    def ortho(a, host=off, dev=fake, seg=fake, elems=seg_elems):
        return lib.lnx_muon_orthogonalize(None if a is None else C.byref(a), None if host is None else host.ctypes.data, dev, seg, elems, None)

    assert ortho(None) != 0 and b"lnx_muon_orthogonalize: args is NULL" in lib.lnx_last_error()
    for field in ("mats", "mats_dev", "tiles_dev", "workspace", "partials"):  # the shared front half, under the caller's name
        a = args()
        setattr(a, field, None)
        assert ortho(a) != 0 and b"lnx_muon_orthogonalize" in lib.lnx_last_error(), field
    a = args()
    a.workspace_bytes -= 1
    assert ortho(a) != 0 and b"workspace bytes" in lib.lnx_last_error()
    a = args()
    mats[1].x_off += 256
    assert ortho(a) != 0 and b"does not match the layout" in lib.lnx_last_error()
    mats[1].x_off -= 256
    assert ortho(args(), host=None) != 0 and b"offset table is NULL" in lib.lnx_last_error()
    assert ortho(args(), dev=None) != 0 and b"offset table is NULL" in lib.lnx_last_error()
    assert ortho(args(), seg=None) != 0 and b"no segment" in lib.lnx_last_error()
    assert ortho(args(), elems=0) != 0 and b"no segment" in lib.lnx_last_error()
    assert ortho(args(), seg=fake + 64) != 0 and b"256-byte aligned" in lib.lnx_last_error()
    assert ortho(args(), elems=48 * 192 + 3968) != 0 and b"outside the segment" in lib.lnx_last_error()  # the second matrix ends 32 elements late
    assert ortho(args(), host=np.asarray([0, -128], dtype=np.int64)) != 0 and b"outside the segment" in lib.lnx_last_error()
    assert ortho(args(), host=np.asarray([0, 48 * 192 + 64], dtype=np.int64)) != 0 and b"not a multiple of 128" in lib.lnx_last_error()
    assert ortho(args(), host=np.asarray([0, 48 * 192 - 128], dtype=np.int64)) != 0 and b"matrices 0 and 1 overlap" in lib.lnx_last_error()
    assert ortho(args(), host=np.asarray([128, 0], dtype=np.int64), elems=48 * 192 + 128) != 0 and b"overlap" in lib.lnx_last_error()

    def table(offs=(0, 9216), numels=(9216, 4000)):
        t = (L.MuonPacked * len(offs))()
        blk = 0
        for d, o, n in zip(t, offs, numels):
            d.p, d.off, d.numel, d.decay, d.step, d.block_start = fake, o, n, 1.0, 0.02, blk
            blk += -(-n // L.MUON_ELEMS)
        return t

    def apply(t, dev=fake, n=None, gathered=fake, elems=13312, world=1, guard=None):
        return lib.lnx_muon_apply_packed(None if t is None else C.addressof(t), dev, len(t) if n is None else n, gathered, elems, world, guard, None)

    t = table()
    assert lib.lnx_muon_apply_packed(None, fake, 2, fake, 13312, 1, None, None) != 0 and b"table is NULL" in lib.lnx_last_error()
    assert apply(t, dev=None) != 0 and b"table is NULL" in lib.lnx_last_error()
    assert apply(t, n=0) != 0 and b"table is NULL or empty" in lib.lnx_last_error()
    for world in (0, -1):
        assert apply(t, world=world) != 0 and b"lnx_muon_apply_packed: world=" in lib.lnx_last_error()
    assert apply(t, gathered=None) != 0 and b"no gathered buffer" in lib.lnx_last_error()
    assert apply(t, elems=13300) != 0 and b"multiple of 128" in lib.lnx_last_error()
    assert apply(t, gathered=fake + 8) != 0 and b"256-byte aligned" in lib.lnx_last_error()
    guard = L.StepGuard()
    assert apply(t, guard=C.pointer(guard)) != 0 and b"guard has no flag" in lib.lnx_last_error()
    assert apply(t, elems=13184) != 0 and b"outside the gathered buffer" in lib.lnx_last_error()  # 9216 + 4000 > 13184
    assert apply(table(offs=(0, 2 * 13312 - 3999)), world=2) != 0 and b"outside the gathered buffer" in lib.lnx_last_error()
    assert apply(table(offs=(0, 9215))) != 0 and b"entries 0 and 1 overlap" in lib.lnx_last_error()
    assert apply(table(offs=(4000, 0), numels=(9216, 4001)), elems=13312) != 0 and b"overlap" in lib.lnx_last_error()
    bad = table()
    bad[1].block_start += 1
    assert apply(bad) != 0 and b"block_start" in lib.lnx_last_error()
    bad = table()
    bad[0].numel = 0
    assert apply(bad) != 0 and b"0 elements" in lib.lnx_last_error()
    bad = table()
    bad[1].p = None
    assert apply(bad) != 0 and b"parameter pointer" in lib.lnx_last_error()
    assert lib.lnx_muon_launches() == before  # refused calls launch nothing


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {"rank": rank}
    try:
        from linnaeus_amd.config import ConfigNode
        from linnaeus_amd.optim import FusedMultiOptimizer, FusedMuon, ShardedFusedMuon, build_optimizer

        model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Linear(16, 4))  # two matrices for Muon, two biases for AdamW
        for flag in (True, False):
            opt = build_optimizer(ConfigNode({"OPTIMIZER": {"NAME": "muon", "MUON": {"USE_DISTRIBUTED": flag}}}), model, max_grad_norm=1.5)
            muon = opt.optimizers["MUON"]
            res[flag] = (type(opt) is FusedMultiOptimizer, type(muon).__name__, getattr(muon, "rank", None), getattr(muon, "world_size", None),
                         isinstance(muon, FusedMuon), opt.max_grad_norm, muon.partition_report()["owner"] if isinstance(muon, ShardedFusedMuon) else None)
    except Exception as e:  # noqa: BLE001 -- reported to the parent, which fails the test with it
        import traceback

        res["error"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
    finally:
        q.put(res)
        dist.destroy_process_group()


def test_build_optimizer_under_two_gloo_ranks():
    """construction only, no step: MUON.USE_DISTRIBUTED builds the sharded optimizer exactly when there are ranks to share with"""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_build_worker, args=(r, world, port, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    res = [q.get(timeout=120) for _ in range(world)]
    for p_ in procs:
        p_.join(60)
        assert p_.exitcode == 0
    for r in res:
        assert "error" not in r, r["error"]
        assert r[True] == (True, "ShardedFusedMuon", r["rank"], 2, True, 1.5, [0, 1])
        assert r[False] == (True, "FusedMuon", None, None, True, 1.5, None)
