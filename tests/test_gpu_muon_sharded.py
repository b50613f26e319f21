"""ShardedFusedMuon on the GPU.  One process simulates a world: W optimizer instances over W clones of the parameters, and a `gather`
seam that does what the all-gather does (rank r's segment lands in part r of every instance's buffer).  FusedMuon gives the same bits
for a matrix alone or in a set, so everything here is held to FusedMuon's exact bits: no tolerance anywhere.  The last test runs two
real ranks over gloo with the default collective."""
import os
import socket
import threading

import pytest
import torch
import torch.multiprocessing as mp

from linnaeus_amd import _lib as L

pytestmark = pytest.mark.gpu

G0 = dict(lr=0.02, weight_decay=0.01, momentum=0.95, nesterov=True, ns_steps=5)
G1 = dict(lr=0.01, weight_decay=0.0, momentum=0.9, nesterov=False, ns_steps=3)
# the small shapes of tests/test_gpu_muon_fused.py: tall, wide, square, 4-D, padding in both dimensions, numel % 4 != 0 (33 x 33, 16 x 49)
TWELVE = [(48, 192), (192, 48), (40, 100), (64, 64), (33, 33), (16, 1, 7, 7), (96, 1, 7, 7), (32, 8, 2, 2), (136, 264), (264, 136), (8, 8), (1, 40)]
WORLDS = [1, 2, 3, 5, 16]  # 16 > 12 matrices: empty ranks
NO_GRAD = (1, 4)           # at the second step, parameter 4 (33 x 33) has no gradient
CLIP = 1.0                 # the gradients' norm is in the hundreds: the clip bites
STEPS = 3


def initial():
    return [torch.randn(*s, generator=torch.Generator().manual_seed(100 + k)) * 0.1 for k, s in enumerate(TWELVE)]


def gradient(step, k):
    return torch.randn(*TWELVE[k], generator=torch.Generator().manual_seed(1000 + 20 * step + k))


def groups(ps):
    return [dict(params=ps[0::2], **G0), dict(params=ps[1::2], **G1)]


def clones(init):
    return [torch.nn.Parameter(t.clone().cuda()) for t in init]


def set_grads(ps, step, poison=None):
    for k, p in enumerate(ps):
        p.grad = None if (step, k) == NO_GRAD else gradient(step, k).cuda()
        if poison == k:
            p.grad.view(-1)[7] = float("inf")


class Handle:
    def __init__(self, fn):
        self.fn = fn

    def wait(self):
        self.fn()


class World:
    """W ranks in one process.  The seam registers the rank's buffer and returns a handle whose wait() copies every rank's segment into
    it: begin_step on all ranks, then finish_step on all ranks, is one step of the world.  A state gather (fp32) asks the peers directly."""

    def __init__(self, world, init, **kw):
        from linnaeus_amd.optim import ShardedFusedMuon

        self.world, self.bufs, self.opts, self.params = world, {}, [], []
        for r in range(world):
            ps = clones(init)
            self.params.append(ps)
            self.opts.append(ShardedFusedMuon(groups(ps), rank=r, world_size=world, gather=lambda out, seg, r=r: self.gather(r, out, seg), **kw))

    def gather(self, r, out, seg):
        if out.dtype == torch.float32:
            for q, o in enumerate(self.opts):
                out.view(self.world, -1)[q].copy_(o._state_segment())
            return None
        self.bufs[r] = out

        def exchange():
            for q in range(self.world):
                if q != r:
                    out.view(self.world, -1)[q].copy_(self.bufs[q].view(self.world, -1)[q])

        return Handle(exchange)

    def set_grads(self, step, poison=None):
        for ps in self.params:
            set_grads(ps, step, poison)

    def step(self):
        for o in self.opts:
            o.begin_step()
        for o in self.opts:
            o.finish_step()


def launches():
    return L.lib().lnx_muon_launches()


@pytest.fixture(scope="module")
def reference():
    """FusedMuon over the scenario, computed once: (initial values, parameters after each step, momentum buffers after each step); read only"""
    from linnaeus_amd.optim import FusedMuon

    init = initial()
    ps = clones(init)
    opt = FusedMuon(groups(ps), max_grad_norm=CLIP)
    after, bufs = [], []
    for s in range(STEPS):
        set_grads(ps, s)
        opt.step()
        after.append([p.detach().clone() for p in ps])
        bufs.append([opt.state[p]["momentum_buffer"].clone() if "momentum_buffer" in opt.state.get(p, {}) else None for p in ps])
    torch.cuda.synchronize()
    assert not torch.equal(after[0][0], init[0].cuda()) and all(torch.isfinite(p).all() for p in after[-1])
    return init, after, bufs, opt.workspace_bytes()


@pytest.mark.parametrize("world", WORLDS)
def test_same_bits_as_fused_muon(reference, world):
    init, after, bufs, _ = reference
    w = World(world, init, max_grad_norm=CLIP)
    flat = [p for g in w.opts[0].param_groups for p in g["params"]]  # the order of partition_report()["owner"]
    owner = [w.opts[0].partition_report()["owner"][next(j for j, x in enumerate(flat) if x is p)] for p in w.params[0]]
    for r in range(world):
        assert [w.opts[r].owns(p) for p in w.params[r]] == [k == r for k in owner]
    assert len(set(owner)) == min(world, len(TWELVE))
    for s in range(STEPS):
        w.set_grads(s)
        w.step()
        for r in range(world):
            for k, p in enumerate(w.params[r]):
                assert torch.equal(p, after[s][k]), (world, s, r, k)
                st = w.opts[r].state.get(p, {})
                if owner[k] == r and bufs[s][k] is not None:
                    assert torch.equal(st["momentum_buffer"], bufs[s][k]), (world, s, r, k)
                else:  # momentum lives on the owner only
                    assert "momentum_buffer" not in st
    k = NO_GRAD[1]
    assert torch.equal(after[NO_GRAD[0]][k], after[NO_GRAD[0] - 1][k])  # the missing gradient: neither decay nor update


def owned_regions(opt):
    """([(parameter, first element in the gathered buffer, numel, group index)] of the matrices this rank owns, seg_elems)"""
    order = opt._all_order()
    owner, off, seg, _ = opt._partition(order)
    return [(p, opt.rank * seg + off[i], p.numel(), gi) for i, (gi, p) in enumerate(order) if owner[i] == opt.rank], seg


def nan_prefill(w):
    """every instance's gathered buffer, allocated ahead of the step and filled with a NaN bit pattern"""
    for o in w.opts:
        seg = o._partition()[2]
        o._gathered = torch.full((w.world * seg,), float("nan"), device="cuda", dtype=torch.bfloat16)
        assert (o._gathered.view(torch.int16) == 0x7FC0).all()


def test_pack_kernel_writes_the_owned_regions_and_nothing_else(reference):
    init, after, _, _ = reference
    world = 3
    w = World(world, init, max_grad_norm=CLIP)
    nan_prefill(w)
    w.set_grads(0)
    for r, o in enumerate(w.opts):
        o.begin_step()
        torch.cuda.synchronize()
        for p, q in zip(w.params[r], init):
            assert torch.equal(p.detach().cpu(), q)  # p is not touched
        bits = o._gathered.view(torch.int16)
        written = torch.zeros_like(bits, dtype=torch.bool)
        regions, seg = owned_regions(o)
        assert regions
        for p, lo, n, gi in regions:
            assert o.rank * seg <= lo and lo + n <= (o.rank + 1) * seg and lo % L.MUON_SEG_ALIGN == 0
            written[lo:lo + n] = True
            k = next(j for j, x in enumerate(w.params[r]) if x is p)
            got = o._gathered[lo:lo + n].view(p.shape)
            assert not torch.isnan(got).any(), TWELVE[k]
            # the O of the unsharded step, re-derived exactly: p_new = fma(-step, O, fl(p decay)).  The product of a bf16 and an fp32 number is
            # exact in fp64, and so is its sum with fl(p decay) unless one term is below 2^-21 of the other; there fp64 rounds 2^29 times
            # finer than fp32.  Rounding that sum once gives the kernel's fp32 result
            g = o.param_groups[gi]
            rows, cols = p.size(0), p.numel() // p.size(0)
            decay = torch.tensor(1 - g["lr"] * g["weight_decay"], dtype=torch.float32, device="cuda")
            step = torch.tensor(g["lr"] * max(1, rows / cols) ** 0.5, dtype=torch.float32, device="cuda")
            pd = init[k].cuda() * decay
            assert torch.equal((pd.double() - step.double() * got.double()).float(), after[0][k]), TWELVE[k]
            # and backwards: (p decay - p_new) / step is O up to the one fp32 rounding of p_new
            rec = (pd.double() - after[0][k].double()) / step.double()
            assert ((rec - got.double()).abs() <= 2.0 ** -24 * after[0][k].abs().double() / step.double() + 1e-12).all(), TWELVE[k]
        assert (bits[~written] == 0x7FC0).all()  # the padding between regions and the other ranks' segments: bit-identical to before
    for o in w.opts:
        o.finish_step()
    for r in range(world):
        for k, p in enumerate(w.params[r]):
            assert torch.equal(p, after[0][k])


def test_nonfinite_guard_skips_on_every_rank_then_steps_as_fused_muon():
    from linnaeus_amd.optim import FusedMuon

    init = initial()
    ref_ps = clones(init)
    ref = FusedMuon(groups(ref_ps), max_grad_norm=CLIP, nonfinite_guard=True)
    world = 3
    w = World(world, init, max_grad_norm=CLIP, nonfinite_guard=True)
    nan_prefill(w)
    set_grads(ref_ps, 0, poison=2)
    ref.step()
    w.set_grads(0, poison=2)
    w.step()
    assert bool(ref.last_step_skipped())
    for r, o in enumerate(w.opts):
        assert bool(o.last_step_skipped()) and int(o.skipped_steps()) == 1
        # nothing was packed, here or on a peer: the exchange copied NaN patterns over NaN patterns
        assert (o._gathered.view(torch.int16) == 0x7FC0).all()
        for p, q in zip(w.params[r], init):
            assert torch.equal(p.detach().cpu(), q)
        for p in w.params[r]:  # the momentum buffers the skipped step created stay zero
            assert not o.state.get(p, {}).get("momentum_buffer", torch.zeros(1)).any()
    set_grads(ref_ps, 1)
    ref.step()
    w.set_grads(1)
    w.step()
    for r, o in enumerate(w.opts):
        assert not bool(o.last_step_skipped())
        for p, q in zip(w.params[r], ref_ps):
            assert torch.equal(p, q)
    assert not torch.equal(ref_ps[0].detach().cpu(), init[0])


@pytest.mark.parametrize("world", [3, 16])
def test_launch_counts_and_workspace(reference, world):
    init, _, _, full_ws = reference
    w = World(world, init)
    w.set_grads(0)
    w.step()
    counts = []
    for o in w.opts:
        before = launches()
        o.begin_step()
        mid = launches()
        o.finish_step()
        counts.append((mid - before, launches() - mid))
    torch.cuda.synchronize()
    total_ws = 0
    for o, (front, back) in zip(w.opts, counts):
        regions, _ = owned_regions(o)
        rep = o.partition_report()
        assert back == 1  # one apply launch over all matrices, whatever the rank owns
        if regions:
            ns = max(o.param_groups[gi]["ns_steps"] for _, _, _, gi in regions)
            assert front == 3 * ns + 3, (o.rank, front, ns)
            from linnaeus_amd.optim import muon_layout

            own = int(muon_layout([(p.size(0), p.numel() // p.size(0)) for p, _, _, _ in regions])[2].workspace_bytes)
            assert o.workspace_bytes() == own == rep["workspace_bytes"]
        else:
            assert front == 0 and o.workspace_bytes() == 0 == rep["workspace_bytes"]  # a rank that owns nothing makes 1 launch per step
        total_ws += o.workspace_bytes()
    assert total_ws == full_ws
    assert sum(1 for f, _ in counts if f == 0) == max(0, world - len(TWELVE))


def test_state_moves_through_the_full_state_dict(reference):
    from linnaeus_amd.optim import FusedMuon

    init, after, bufs, _ = reference
    world = 3
    w = World(world, init, max_grad_norm=CLIP)
    ref_ps = clones(init)
    ref = FusedMuon(groups(ref_ps), max_grad_norm=CLIP)
    for s in range(2):
        set_grads(ref_ps, s)
        ref.step()
        w.set_grads(s)
        w.step()
    want = ref.state_dict()
    fulls = [o.full_state_dict() for o in w.opts]
    for got in fulls:
        assert got["param_groups"] == want["param_groups"] and sorted(got["state"]) == sorted(want["state"])
        for k in want["state"]:
            assert set(got["state"][k]) == {"momentum_buffer"} and torch.equal(got["state"][k]["momentum_buffer"], want["state"][k]["momentum_buffer"])
    for o in w.opts:  # the local shard: the owned subset
        local = o.state_dict()["state"]
        assert set(local) <= set(want["state"]) and len(local) < len(want["state"])
    # fresh instances at the parameters of step 2 take the full dict, keep their part, and make FusedMuon's third step
    now = [t.cpu() for t in after[1]]
    fresh = World(world, now, max_grad_norm=CLIP)
    for o in fresh.opts:
        o.load_state_dict(fulls[1])
    fresh.set_grads(2)
    fresh.step()
    for r in range(world):
        for k, p in enumerate(fresh.params[r]):
            assert torch.equal(p, after[2][k]), (r, k)
    assert sum(len(o.state) for o in fresh.opts) == len(TWELVE)


def test_multi_optimizer_with_a_sharded_muon_matches_the_unsharded_one():
    """{"MUON": ShardedFusedMuon, "ADAMW": FusedAdamW} under a shared clip and the guard, one thread per rank so that every rank's
    FusedMultiOptimizer.step() runs whole: begin_step, the AdamW launch, finish_step (the seam's wait() is the rendezvous)."""
    from linnaeus_amd.optim import FusedAdamW, FusedMultiOptimizer, FusedMuon, ShardedFusedMuon

    init = initial()
    vec_init = [torch.randn(n, generator=torch.Generator().manual_seed(500 + n)) for n in (7, 300, 4097)]
    world = 2

    def vec_grads(vs, s):
        for j, v in enumerate(vs):
            v.grad = torch.randn(v.shape, generator=torch.Generator().manual_seed(700 + 10 * s + j)).cuda()

    ref_ps, ref_vs = clones(init), clones(vec_init)
    ref = FusedMultiOptimizer({"MUON": FusedMuon(groups(ref_ps)), "ADAMW": FusedAdamW(ref_vs, lr=1e-2)}, max_grad_norm=CLIP, nonfinite_guard=True)
    barrier = threading.Barrier(world, timeout=120)
    bufs, multis, params = {}, [], []

    def seam(r, out, seg):
        bufs[r] = out

        def exchange():
            barrier.wait()  # every rank has queued its orthogonalisation (one device stream: the copies below are ordered behind it)
            for q in range(world):
                if q != r:
                    out.view(world, -1)[q].copy_(bufs[q].view(world, -1)[q])
            barrier.wait()  # nobody packs the next step into a segment a peer still has to copy

        return Handle(exchange)

    for r in range(world):
        ps, vs = clones(init), clones(vec_init)
        params.append((ps, vs))
        muon = ShardedFusedMuon(groups(ps), rank=r, world_size=world, gather=lambda out, seg, r=r: seam(r, out, seg))
        multis.append(FusedMultiOptimizer({"MUON": muon, "ADAMW": FusedAdamW(vs, lr=1e-2)}, max_grad_norm=CLIP, nonfinite_guard=True))
    for s in range(STEPS):
        poison = 2 if s == 1 else None  # the second step is skipped by the guard, on every rank and in both sub-optimizers
        set_grads(ref_ps, s, poison)
        vec_grads(ref_vs, s)
        ref.step()
        errors = []

        def run(r):
            try:
                torch.cuda.set_device(0)
                multis[r].step()
            except BaseException as e:  # noqa: BLE001 -- re-raised in the test's thread
                errors.append(e)
                barrier.abort()

        for ps, vs in params:
            set_grads(ps, s, poison)
            vec_grads(vs, s)
        threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        if errors:  # the cause, not the broken rendezvous it left behind on the other rank
            raise next((e for e in errors if not isinstance(e, threading.BrokenBarrierError)), errors[0])
        torch.cuda.synchronize()
        assert bool(ref.last_step_skipped()) == (s == 1)
        for r in range(world):
            assert bool(multis[r].last_step_skipped()) == (s == 1)
            for p, q in zip(params[r][0] + params[r][1], ref_ps + ref_vs):
                assert torch.equal(p, q), (s, r)
    assert not torch.equal(ref_ps[0].detach().cpu(), init[0]) and not torch.equal(ref_vs[0].detach().cpu(), vec_init[0])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    res = {"rank": rank}
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from linnaeus_amd.optim import FusedMuon, ShardedFusedMuon

        init = initial()
        ps = clones(init)
        opt = ShardedFusedMuon(groups(ps), max_grad_norm=CLIP)  # rank, world size and the collective: the default process group's
        res["rank_world"] = (opt.rank, opt.world_size)
        ref_ps = clones(init) if rank == 0 else None
        ref = FusedMuon(groups(ref_ps), max_grad_norm=CLIP) if rank == 0 else None
        for s in range(STEPS):
            set_grads(ps, s)
            opt.step()
            if rank == 0:
                set_grads(ref_ps, s)
                ref.step()
        torch.cuda.synchronize()
        flat = torch.cat([p.detach().flatten() for p in ps])
        others = [torch.empty_like(flat) for _ in range(world)]
        dist.all_gather(others, flat)
        res["ranks_agree"] = all(torch.equal(flat, o) for o in others)
        res["finite"] = bool(torch.isfinite(flat).all())
        res["moved"] = not torch.equal(flat.cpu(), torch.cat([t.flatten() for t in init]))
        if rank == 0:
            res["equals_fused_muon"] = all(torch.equal(p, q) for p, q in zip(ps, ref_ps))
        res["owned_state"] = len(opt.state)
        res["collective"] = opt.collective
    except Exception as e:  # noqa: BLE001 -- reported to the parent, which fails the test with it
        import traceback

        res["error"] = f"{type(e).__name__}: {e}\n{traceback.format_exc()}"
    finally:
        q.put(res)
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_real_ranks_over_gloo():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p_ in procs:
        p_.start()
    res = [q.get(timeout=240) for _ in range(world)]
    for p_ in procs:
        p_.join(60)
        assert p_.exitcode == 0
    for r in res:
        assert "error" not in r, r["error"]
    for r in sorted(res, key=lambda r: r["rank"]):
        print(f"[sharded muon, two ranks] rank {r['rank']}: collective {r['collective']}, {r['owned_state']} momentum buffers")
        assert r["collective"] in ("all_gather_into_tensor", "all_gather")
        assert r["rank_world"] == (r["rank"], world)
        assert r["finite"] and r["moved"]
        assert r["ranks_agree"], "the ranks hold different parameters after three sharded steps"
        assert 0 < r["owned_state"] < len(TWELVE)
    assert sorted(res, key=lambda r: r["rank"])[0]["equals_fused_muon"], "rank 0 differs from an unsharded FusedMuon"
    assert sum(r["owned_state"] for r in res) == len(TWELVE)
