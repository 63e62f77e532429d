"""Cost of the league results (VecCatanEnv.enable_league_stats) on the deferred rollout: the same handle runs the bench's loop
(catan_random_rollout_deferred, 65 536 games, window 32) alternately with the tally off and on, `--rounds` times each; env-steps/s from the
games' own decision counters, as bench.py counts them.  usage: bench_league_stats.py [--envs N] [--steps K] [--window W] [--rounds R] [--nets K]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nets", type=int, default=8, help="opponent nets in play (tools/train.py --league)")
    ap.add_argument("--preroll", type=int, default=2048, help="untimed passes that mix the games' ages")
    args = ap.parse_args()
    import torch
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv(args.envs, seed=0)
    g = torch.Generator().manual_seed(0)
    slot = torch.stack([torch.randperm(4, generator=g) for _ in range(args.envs)])
    net = torch.randint(0, args.nets, (args.envs, 3), generator=g)
    env.random_rollout_deferred(args.preroll, args.window)
    torch.cuda.synchronize()
    rows = []
    for r in range(args.rounds):
        for on in (False, True):
            env.enable_league_stats(slot if on else None, net if on else None, args.nets, on=on)
            env.random_rollout_deferred(256, args.window)                  # warm-up in the mode that is timed
            c0 = int(env.policy_counters().sum())
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.random_rollout_deferred(args.steps, args.window)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            steps = int(env.policy_counters().sum()) - c0
            row = {"round": r, "league_stats": on, "env_steps_per_s": steps / dt, "us_per_pass": dt / args.steps * 1e6, "env_steps": steps}
            if on:
                t = env.league_stats()
                row["games_tallied"] = int(t[-1, 1])                        # (warm-up + timed passes)
                assert int(t[:-1, 1].sum()) == 3 * row["games_tallied"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    off = sorted(x["env_steps_per_s"] for x in rows if not x["league_stats"])
    on = sorted(x["env_steps_per_s"] for x in rows if x["league_stats"])
    print(json.dumps({"envs": args.envs, "passes": args.steps, "window": args.window, "nets": args.nets, "off_min_median_max": [off[0], off[len(off) // 2], off[-1]],
                      "on_min_median_max": [on[0], on[len(on) // 2], on[-1]], "on_over_off_median": on[len(on) // 2] / off[len(off) // 2]}))
    assert env.invalid_action_count() == 0


if __name__ == "__main__":
    main()
