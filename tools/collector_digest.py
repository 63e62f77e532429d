"""Digests of what small rollout collectors leave behind, to compare two versions of the host code bit for bit: run it once per
version, each in its own process (`--root` = the checkout whose package is imported), and diff the two outputs.  Per collector
and gather_rollouts: a sha256 of every storage tensor, of the four counters, of racc / done_since / pending_obs and of
env.export_state(), then games_complete, iters, bucket_log and env.invalid_action_count()."""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--only", type=int, default=None, help="index of the one collector to run")
ap.add_argument("--gathers", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from settlers_of_catan_rl_amd.env import VecCatanEnv  # noqa: E402
from settlers_of_catan_rl_amd.policy import CatanPolicy  # noqa: E402
from settlers_of_catan_rl_amd.rollout import RolloutCollector  # noqa: E402

N, T = 2048, 6
BF16 = dict(autocast_dtype=torch.bfloat16, graph_act=True)


def league(col):
    torch.manual_seed(1)
    nets = [CatanPolicy().cuda() for _ in range(3)]
    col.set_opponents(nets, torch.randint(0, 3, (N, 3), generator=torch.Generator().manual_seed(5)))


# (name, env keywords, policy keywords, collector keywords, set-up of the collector, max_iters)
CONFIGS = [
    ("buckets, default deferred window", dict(dense_reward=True), {}, BF16, None, None),
    ("buckets, catan_step", {}, {}, dict(BF16, deferred_window=0), None, None),
    ("act_buckets 256/512/1024, deferred W=8", {}, {}, dict(BF16, act_buckets=(256, 512, 1024), deferred_window=8), None, None),
    ("league of three nets, captured passes", {}, {}, BF16, league, None),
    ("league of three nets, eager passes", {}, {}, dict(BF16, graph_act=False), league, None),
    ("tensor-operation bookkeeping", {}, {}, BF16, lambda col: setattr(col, "fused_bookkeeping", False), None),
    ("LSTM policy", {}, dict(include_lstm=True), dict(autocast_dtype=None), None, None),
    ("max_iters=5, deferred", {}, {}, BF16, None, 5),
]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()).hexdigest()[:16]


for i, (name, ekw, pkw, ckw, setup, max_iters) in enumerate(CONFIGS):
    if args.only is not None and i != args.only:
        continue
    torch.manual_seed(0)
    env = VecCatanEnv(N, seed=3 + i, **ekw)
    env.random_rollout(0, 1500)
    col = RolloutCollector(env, CatanPolicy(**pkw).cuda(), T, seed=i, **ckw)
    if setup is not None:
        setup(col)
    for k in range(args.gathers):
        st = col.gather_rollouts(max_iters=max_iters)
        what = {n: getattr(st, n) for n in ("obs_f", "lists", "lens", "masks", "rewards", "actions", "action_log_probs", "action_masks", "hidden")}
        what.update({n: getattr(col, n) for n in ("n_obs", "n_msk", "n_act", "n_rew", "racc", "done_since", "pending_obs")}, state=env.export_state())
        print(f"[{i}] {name} | gather {k} | " + " ".join(f"{n}={sha(t)}" for n, t in what.items() if t is not None))
        print(f"[{i}] {name} | gather {k} | games_complete={st.games_complete} iters={col.iters} bucket_log={getattr(col, 'bucket_log', None)} "
              f"invalid={env.invalid_action_count()}", flush=True)
        col.after_rollouts()
    col.close()
    del col, st, env
    torch.cuda.empty_cache()
