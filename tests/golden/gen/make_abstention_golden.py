#!/usr/bin/env python3
"""Generate tests/golden/abstention.npz from the reference's own reward functions (linnaeus/rl_env/reward_functions.py, loaded by path,
unmodified) and, where it imports, its compute_gae_and_returns (linnaeus/rl_train_abstention.py).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_abstention_golden.py <linnaeus checkout>

rl_train_abstention.py imports the whole training stack and `gym` at module level (and calls sys.exit when one import fails).  It is
tried with the stand-ins under _stubs/ (a `gym` of our own among them); `gae_from_reference` records whether that worked.  When it
did not, the GAE arrays are absent and tests/test_abstention_host.py checks the recursion against tests/abstention_ref.py only.

Writes numbers only:
  gt, pred            int64 [216, 3]: every combination of ground truth in {None, 1} and prediction in {None, 1, 2} over three ranks
                      (-1 = None): all five outcomes at every rank position
  table_<i>, values_<i>   the constructor arguments of SimpleAbstentionReward / EpisodeOutcomeReward, i = 0 the defaults, i = 1 others
  simple_list_<i>, outcome_list_<i>   float64 [216]: compute_reward in the list form {"k": [p0, p1, p2]} the docstrings describe
  simple_dict_<i>, outcome_dict_<i>   float64 [216]: compute_reward in the form {rank: [label]} the environment and verifier pass
                      (finding F-a: only the first rank is counted)
  gae_*               (with gae_from_reference = 1) seeded episodes: rewards, values, dones, gamma, lambda -> advantages, returns
"""
import importlib.util
import itertools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
if len(sys.argv) != 2 or not os.path.isfile(os.path.join(sys.argv[1], "linnaeus", "rl_env", "reward_functions.py")):
    sys.exit(f"usage: {sys.argv[0]} <path of a linnaeus checkout>")
REF = os.path.abspath(sys.argv[1])
sys.path[:0] = [os.path.join(HERE, "_stubs"), REF]
sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_reward_functions", os.path.join(REF, "linnaeus", "rl_env", "reward_functions.py"))
rf = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rf)

TABLES = [(1.0, 0.5, -1.0, -0.5, -1.0), (0.7, 0.3, -1.1, -0.4, -0.9)]  # the argument order of SimpleAbstentionReward
VALUES = [(1.0, -1.0), (2.5, -0.3)]
KEYS = ("family", "genus", "species")


def label(v):
    return None if v < 0 else int(v)


def main():
    per_rank = [(g, p) for g in (-1, 1) for p in (-1, 1, 2)]
    combos = list(itertools.product(per_rank, repeat=3))
    gt = np.array([[c[r][0] for r in range(3)] for c in combos], dtype=np.int64)
    pred = np.array([[c[r][1] for r in range(3)] for c in combos], dtype=np.int64)
    out = {"gt": gt, "pred": pred}
    for i, (table, values) in enumerate(zip(TABLES, VALUES)):
        simple, outcome = rf.SimpleAbstentionReward(*table), rf.EpisodeOutcomeReward(*values)
        out[f"table_{i}"], out[f"values_{i}"] = np.array(table), np.array(values)
        for name, fn in (("simple", simple), ("outcome", outcome)):
            as_list, as_dict = [], []
            for g, p in zip(gt, pred):
                as_list.append(fn.compute_reward({"k": [label(v) for v in p]}, {"k": [label(v) for v in g]}))
                as_dict.append(fn.compute_reward({k: [label(v)] for k, v in zip(KEYS, p)}, {k: [label(v)] for k, v in zip(KEYS, g)}))
            out[f"{name}_list_{i}"], out[f"{name}_dict_{i}"] = np.array(as_list, dtype=np.float64), np.array(as_dict, dtype=np.float64)

    gae = None
    try:
        import linnaeus.rl_train_abstention as rta

        gae = rta.compute_gae_and_returns
    except BaseException as e:  # (SystemExit included: the module exits when an import fails)
        print(f"rl_train_abstention.py does not import here ({type(e).__name__}: {e}); GAE is checked against the restatement only")
    out["gae_from_reference"] = np.array(0 if gae is None else 1)
    if gae is not None:
        rng = np.random.default_rng(20251021)
        lengths = [1, 2, 3, 5, 8, 4]
        rewards, values, dones = [], [], []
        for n in lengths:  # complete episodes back to back, as a rollout buffer holds them
            r = np.zeros(n)
            r[-1] = rng.choice([-1.0, -0.5, 0.5, 1.0, 2.5])
            d = np.zeros(n)
            d[-1] = 1.0
            rewards.append(r)
            values.append(np.full(n, rng.normal()))
            dones.append(d)
        rewards, values, dones = (np.concatenate(v).astype(np.float64) for v in (rewards, values, dones))
        adv, ret = gae(rewards, values, dones, 123.0, 0.99, 0.95)  # last_value is multiplied by 1 - done = 0
        out.update(gae_lengths=np.array(lengths), gae_rewards=rewards, gae_values=values, gae_dones=dones, gae_gamma=np.array(0.99),
                   gae_lambda=np.array(0.95), gae_adv=adv, gae_ret=ret)
    path = os.path.join(REPO, "tests", "golden", "abstention.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(combos)} cases, gae_from_reference={int(out['gae_from_reference'])}")


if __name__ == "__main__":
    main()
