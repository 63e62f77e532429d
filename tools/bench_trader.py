"""The rule-based "trader" player (scripted.TraderPolicy, k_sample_trader) measured: (1) time per call of
catan_sample_scripted_actions_style with style 1 against style 0 (the builder's kernel) on the same states (hipEvents around `--reps`
back-to-back calls, `--rounds` alternating rounds, warm-up first; the states are a mix of game ages reached by the trader, the builder
and the uniform-random sampler taking turns); (2) evaluation games with the seeds and seat orders of the builder's strength test
(tests/test_gpu_scripted.py): one trader against three uniform-random players, and two traders against two builders, with the
trader's counter block (catan_scripted_trade_counts) of those games.
Appends one JSON line per measurement, with the commit they were measured on, to `--out`.

As in tools/bench_scripted.py, each call of (1) goes through Python and ctypes: where the figure is close to host_issue_us it is the
host's launch cost and only bounds the kernel's time from above.

With --parent-library (a libcatan_hip.so built from the parent commit) it first runs bench.py `--bench-pairs` times under each library,
alternating, every run a fresh process, as tools/bench_teacher.py does: with the style unused the change passes where its mean lies
inside the spread (min..max) of the parent's own runs, or above it.

usage: bench_trader.py [--envs N] [--episodes E] [--reps R] [--rounds K] [--skip-games] [--skip-calls] [--out FILE] [--commit TEXT]
                       [--parent-library libcatan_hip.so --bench-pairs B]"""
import argparse
import json
import os
import random
import sys

import parent_compare as pc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-library")
    ap.add_argument("--bench-pairs", type=int, default=6)
    ap.add_argument("--bench-steps", type=int, default=4096)
    ap.add_argument("--bench-warmup", type=int, default=256)
    ap.add_argument("--bench-child", action="store_true")
    ap.add_argument("--library")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--episodes", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mix-steps", type=int, default=400, help="untimed steps that spread the games over the phases of play")
    ap.add_argument("--max-steps", type=int, default=2500)
    ap.add_argument("--skip-games", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(pc.ROOT, "profiles", "trader_policy_bench.txt"))
    ap.add_argument("--commit", type=str, default=None, help="the commit of this tree (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if args.bench_child:
        return pc.bench_py_child(args.library, args.bench_steps, args.bench_warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    if args.parent_library:                 # first, while this process has not touched the device
        pc.bench_py_section(args, out, "style", __file__)
    import numpy as np
    import torch
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy, TraderPolicy

    out.write("\nRule-based trader player (k_sample_trader, scripted.TraderPolicy): measurements of tools/bench_trader.py\n"
              "commit: {}\ndevice: {}\ncommand: bench_trader.py {}\n"
              "One JSON line per measurement.  us_per_call as in profiles/scripted_policy_bench.txt (hipEvents around `reps` calls through\n"
              "Python and ctypes; close to host_issue_us = launch-bound).  win shares: the share of games won by the policies named first in\n"
              "`measurement`; trade_counts: catan_scripted_trade_counts over those games.\n\n".format(
                  args.commit or pc.commit_of_tree(), torch.cuda.get_device_name(0), " ".join(a for a in sys.argv[1:] if not a.startswith("--commit"))))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    if not args.skip_calls:
        call_times(args, emit, VecCatanEnv, torch)
    if not args.skip_games:
        games(args, emit, VecCatanEnv, ScriptedPolicy, TraderPolicy, ev, np, torch)


def call_times(args, emit, VecCatanEnv, torch):
    """(1) the two styles on the same states"""
    env = VecCatanEnv(args.envs, seed=0)
    g = torch.arange(args.envs, device=env.device)
    for s in range(args.mix_steps):
        t, b, r = env.sample_scripted_actions(style="trader"), env.sample_scripted_actions(), env.sample_random_actions(s)
        mix = ((g + s) % 4)[:, None]
        env.step(torch.where(mix == 0, r, torch.where(mix == 1, b, t)))
    env.scripted_trade_counts(reset=True)
    buf = torch.empty((args.envs, 18), dtype=torch.int32, device=env.device)
    calls = {"trader": lambda: env.sample_scripted_actions(out=buf, style="trader"), "builder": lambda: env.sample_scripted_actions(out=buf)}
    t = pc.event_call_times(calls, args.reps, args.rounds)
    counts = env.scripted_trade_counts()
    per_call = {k: v / (10 + args.rounds * args.reps) for k, v in counts.items()}
    emit({"measurement": "us_per_call", "envs": args.envs, "reps": args.reps, "rounds": args.rounds,
          "trader_min_median_max": t["trader"]["device_us"], "builder_min_median_max": t["builder"]["device_us"],
          "trader_host_issue_us_min_median_max": t["trader"]["host_issue_us"], "builder_host_issue_us_min_median_max": t["builder"]["host_issue_us"],
          "trader_decisions_per_call_on_these_states": per_call})
    assert env.invalid_action_count() == 0


def games(args, emit, VecCatanEnv, ScriptedPolicy, TraderPolicy, ev, np, torch):
    """(2) evaluation games: the seeds and seat orders of tests/test_gpu_scripted.py's strength test"""
    n = args.episodes
    trader, builder, rnd = TraderPolicy(), ScriptedPolicy(), pc.UniformRandom()
    for name, seats, first in (("trader_vs_3_uniform_random", [trader, rnd, rnd, rnd], 1),
                               ("builder_vs_3_uniform_random", [builder, rnd, rnd, rnd], 1),
                               ("2_traders_vs_2_builders", [trader, trader, builder, builder], 2),
                               ("4_traders", [trader] * 4, 4)):
        e = VecCatanEnv(n, seed=21, auto_reset=False)
        for p in {id(x): x for x in seats}.values():
            p.rebind(e)
        res = ev.run_evaluation_episodes(e, seats, ev.sample_orders(n, random.Random(3)), max_steps=args.max_steps)
        assert e.invalid_action_count() == 0
        w = res["winner"]
        c = e.scripted_trade_counts()
        emit({"measurement": name, "episodes": n, "env_seed": 21, "orders_seed": 3, "max_steps": args.max_steps,
              "win_share_of_the_first_%d" % first: float(np.mean((w >= 0) & (w < first))), "fair_share": first / 4.0,
              "draws": float(np.mean(w == -1)), "mean_game_steps": float(np.mean(res["game_steps"])),
              "trade_counts": c, "accepts_per_game": c["accepts"] / n, "builder_fallback_count": e.scripted_fallback_count()})


if __name__ == "__main__":
    main()
