#!/usr/bin/env python3
"""What the abstention phase costs after the forward: rollout (lnx_abstain_act), advantages (lnx_ppo_advantages) and one PPO minibatch
(lnx_ppo_loss_fwd + lnx_ppo_loss_bwd through autograd), against the torch composition of the same definitions (LNX_ABSTENTION=0) in
the same process.

Two sizes, batch 256, sequential mode, fp32 logits as the plan returns them, ranks coarsest first:
  heads      the four heads of mFormerV1_sm: 20 / 80 / 300 / 1000 classes
  taxonomy   100 / 600 / 3 000 / 10 000 classes (the taxonomy of profiles/hier_refine_bench.log)
Logits are seeded normal draws times 2 with a boosted true class and an abstain class at probability 0.2 (episodes of every length).
Per leg and step: --warmup calls, then --iters calls between two device synchronisations on the host clock; the two legs alternate
--repeats times in one process so that drift hits both alike; the median and all repeats are reported.  These are call times, the
host's share (allocations, the autograd Function, the launches) inside.  Also reported: the launches each step made (the library's
own counter) and the largest differences between the two legs: the rollouts on the same logits and uniforms, the advantages and the
loss on the device leg's rollout.  One JSON line at the end."""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import torch  # noqa: E402

SIZES = {"heads": [20, 80, 300, 1000], "taxonomy": [100, 600, 3000, 10000]}  # decision order: coarsest first


def make_inputs(classes, B, dev, seed):
    g = torch.Generator().manual_seed(seed)
    logits, targets = [], []
    for C_ in classes:
        x = torch.randn(B, C_, generator=g) * 2.0
        true = torch.randint(1, C_, (B,), generator=g)
        x[torch.arange(B), true] += math.log(C_) + 3.0
        x[:, 0] = torch.logsumexp(x[:, 1:], dim=1) + math.log(0.25)  # abstain (class 0) at probability 0.2
        t = true.clone()
        t[torch.rand(B, generator=g) < 0.3] = 0
        logits.append(x.to(dev))
        targets.append(t.to(dev))
    return logits, targets, torch.rand(B, len(classes), generator=g).to(dev), torch.randn(B, generator=g).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", default="sequential", choices=["sequential", "multitask"])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_abstention.py needs the MI355X: a time taken elsewhere says nothing about it")
    from linnaeus_amd import rl

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    B, mode = args.batch, args.mode
    reward = rl.AbstentionReward("simple", "all")
    result = {"device": torch.cuda.get_device_name(0), "batch": B, "mode": mode, "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats}

    for size, classes in SIZES.items():
        logits, targets, u, value = make_inputs(classes, B, dev, 42)
        R = len(classes)

        def steps(fused, rolled=None):
            os.environ["LNX_ABSTENTION"] = "1" if fused else "0"
            own = rl.act(logits, targets, u, mode, False, reward)
            acted = rolled or own  # the later steps of both legs work on the SAME rollout, so that their results can be compared
            adv, ret, _ = rl.advantages(acted.reward, value, acted.length, mode, R)
            leaves = [x.clone().requires_grad_(True) for x in logits]
            v = value.clone().requires_grad_(True)

            def minibatch():
                for t in leaves + [v]:
                    t.grad = None
                total, stats = rl.ppo_loss(leaves, v, acted.actions, acted.taken, acted.logp, adv, ret, mode, 0.2, 0.5, 0.01)
                total.backward()
                return total

            return {"rollout": lambda: rl.act(logits, targets, u, mode, False, reward),
                    "advantages": lambda: rl.advantages(acted.reward, value, acted.length, mode, R),
                    "minibatch": minibatch}, (own, adv, ret, leaves, v)

        legs = {"device": steps(True)}
        legs["torch_composition"] = steps(False, rolled=legs["device"][1][0])
        # the two legs on the same inputs
        (fa, fadv, fret, fl, fv), (ta, tadv, tret, tl, tv) = legs["device"][1], legs["torch_composition"][1]
        os.environ["LNX_ABSTENTION"] = "1"
        f_total = float(legs["device"][0]["minibatch"]())
        before = rl.launches()
        legs["device"][0]["rollout"]()
        n_act = rl.launches() - before
        legs["device"][0]["advantages"]()
        n_adv = rl.launches() - before - n_act
        legs["device"][0]["minibatch"]()
        n_loss = rl.launches() - before - n_act - n_adv
        os.environ["LNX_ABSTENTION"] = "0"
        t_total = float(legs["torch_composition"][0]["minibatch"]())
        same = fa.actions == ta.actions  # (a draw within rounding of a class boundary of the running sum may fall either way)
        agree = {"decisions": int(same.numel()), "decisions_with_another_action": int((~same).sum()),
                 "largest_class_distance": int((fa.actions - ta.actions).abs().max()),
                 "max_abs_logp_difference_where_equal": float(((fa.logp - ta.logp) * same).abs().max()),
                 "max_abs_adv_difference": float((fadv - tadv).abs().max()),
                 "total_loss": [f_total, t_total],
                 "max_abs_dlogits_difference": max(float((a.grad - b.grad).abs().max()) for a, b in zip(fl, tl)),
                 "max_abs_dvalue_difference": float((fv.grad - tv.grad).abs().max())}

        rows = {leg: {s: [] for s in ("rollout", "advantages", "minibatch")} for leg in legs}
        for leg, (fns, _) in legs.items():
            os.environ["LNX_ABSTENTION"] = "1" if leg == "device" else "0"
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
        torch.cuda.synchronize()
        for r in range(args.repeats):
            for leg, (fns, _) in legs.items():
                os.environ["LNX_ABSTENTION"] = "1" if leg == "device" else "0"
                for step, fn in fns.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        fn()
                    torch.cuda.synchronize()
                    us = (time.perf_counter() - t0) / args.iters * 1e6
                    rows[leg][step].append(round(us, 1))
                    print(f"[bench_abstention] {size} B={B} classes={classes} repeat {r} {leg} {step}: {us:.1f} us / call", file=sys.stderr, flush=True)
        med = {leg: {s: sorted(v)[len(v) // 2] for s, v in d.items()} for leg, d in rows.items()}
        logit_mb = sum(x.numel() * 4 for x in logits) / 1e6
        result[size] = {"classes": classes, "logits_mb": round(logit_mb, 2), "median_us": med, "all_us": rows,
                        "torch_over_device": {s: round(med["torch_composition"][s] / med["device"][s], 2) for s in med["device"]},
                        "launches": {"rollout": n_act, "advantages": n_adv, "minibatch_forward_plus_backward": n_loss}, "legs_agree": agree}
    os.environ.pop("LNX_ABSTENTION", None)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
