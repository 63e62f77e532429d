"""The rule-based baseline player (scripted.ScriptedPolicy, k_sample_scripted) measured: (1) time per call of
catan_sample_scripted_actions against catan_sample_random_actions on the same states (hipEvents around `--reps` back-to-back calls,
`--rounds` alternating rounds, warm-up first; the states are a mix of game ages reached by the bot playing two moves in three);
(2) wall time of evaluation.run_evaluation_protocol's games for `--episodes` episodes against three ScriptedPolicy and against three
copies of a random-initialised net; (3) the bot's win share against three uniform-random players (also in the configuration of
tests/test_gpu_scripted.py's strength test) and against three copies of a fresh net.
Prints one JSON line per measurement and writes them, with the commit they were measured on, to `--out`.

What (1) is and is not: each call goes through Python and ctypes, so the events bracket `reps` host launches as well as `reps` kernels.
Where the kernel is shorter than the host's time to issue a call, the figure is the host's launch cost and not the kernel's time; the
tool therefore also reports the host's issue time per call (`host_issue_us`: the same loop timed on the host without waiting for the
device).  A per-call figure close to `host_issue_us` is launch-bound and only bounds the kernel from above.

usage: bench_scripted.py [--envs N] [--episodes E] [--reps R] [--rounds K] [--skip-protocol] [--out FILE] [--commit TEXT]"""
import argparse
import json
import os
import random
import sys
import time

import parent_compare as pc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--episodes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--mix-steps", type=int, default=400, help="untimed steps that spread the games over the phases of play")
    ap.add_argument("--max-steps", type=int, default=2500)
    ap.add_argument("--skip-protocol", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(pc.ROOT, "profiles", "scripted_policy_bench.txt"))
    ap.add_argument("--commit", type=str, default=None, help="the commit of this tree (default: git rev-parse HEAD)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w")
    out.write("Rule-based baseline player (k_sample_scripted, scripted.ScriptedPolicy): measurements of tools/bench_scripted.py\n"
              "commit: {}\ndevice: {}\ncommand: bench_scripted.py {}\n"
              "One JSON line per measurement.  us_per_call: hipEvents around `reps` back-to-back calls through Python and ctypes, so the\n"
              "figure holds the host's launch cost too; where it is close to host_issue_us (the same loop timed on the host alone) the call\n"
              "is launch-bound and the figure only bounds the kernel's time from above.  wall_s: the games of one protocol entry\n"
              "(run_evaluation_episodes, bf16 nets), env creation left out.  policy0_win_share: the share of games won by the first policy\n"
              "named in `measurement`; a player no better than the other three wins 0.25.\n\n".format(
                  args.commit or pc.commit_of_tree(), torch.cuda.get_device_name(0), " ".join(a for a in sys.argv[1:] if not a.startswith("--commit"))))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    # ---- (1) the two samplers on the same states
    env = VecCatanEnv(args.envs, seed=0)
    g = torch.arange(args.envs, device=env.device)
    for s in range(args.mix_steps):
        a, r = env.sample_scripted_actions(), env.sample_random_actions(s)
        env.step(torch.where((((g + s) % 3) == 0)[:, None], r, a))
    buf = torch.empty((args.envs, 18), dtype=torch.int32, device=env.device)
    calls = {"scripted": lambda: env.sample_scripted_actions(out=buf), "random": lambda: env.sample_random_actions(7, out=buf)}
    t = pc.event_call_times(calls, args.reps, args.rounds)
    types = torch.bincount(env.sample_scripted_actions()[:, 0].long(), minlength=13).tolist()
    emit({"measurement": "us_per_call", "envs": args.envs, "reps": args.reps, "rounds": args.rounds,
          "scripted_min_median_max": t["scripted"]["device_us"], "random_min_median_max": t["random"]["device_us"],
          "scripted_host_issue_us_min_median_max": t["scripted"]["host_issue_us"], "random_host_issue_us_min_median_max": t["random"]["host_issue_us"],
          "bot_action_types_on_these_states": types, "fallback_count": env.scripted_fallback_count()})
    assert env.invalid_action_count() == 0
    del env
    if args.skip_protocol:
        return

    # ---- (2), (3) evaluation games
    torch.manual_seed(0)
    net = CatanPolicy().cuda().eval()

    def games(first, others, n, seed, order_seed, autocast):
        e = VecCatanEnv(n, seed=seed, auto_reset=False)
        for p in {id(x): x for x in [first] + others}.values():
            if hasattr(p, "rebind"):
                p.rebind(e)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.run_evaluation_episodes(e, [first] + others, ev.sample_orders(n, random.Random(order_seed)), max_steps=args.max_steps,
                                         autocast_dtype=autocast)
        torch.cuda.synchronize()
        assert e.invalid_action_count() == 0
        return res, time.perf_counter() - t0

    bot, rnd, n = ScriptedPolicy(), pc.UniformRandom(), args.episodes
    for name, first, other, m, seed, order_seed, ac in (
            ("net_vs_3_scripted", net, bot, n, 100, 100, torch.bfloat16),
            ("net_vs_3_random_init_nets", net, CatanPolicy().cuda().eval(), n, 100, 100, torch.bfloat16),
            ("scripted_vs_3_uniform_random", bot, rnd, n, 100, 100, torch.bfloat16),
            ("scripted_vs_3_fresh_nets", bot, net, n, 100, 100, torch.bfloat16),
            # the games of tests/test_gpu_scripted.py::test_the_bot_beats_three_uniform_random_players (its bound: > 0.3457, draws <= 0.05)
            ("scripted_vs_3_uniform_random_as_in_the_strength_test", bot, rnd, 512, 21, 3, None)):
        res, dt = games(first, [other] * 3, m, seed, order_seed, ac)
        emit({"measurement": name, "episodes": m, "env_seed": seed, "orders_seed": order_seed, "max_steps": args.max_steps, "wall_s": dt,
              "policy0_win_share": float(np.mean(res["winner"] == 0)), "draws": float(np.mean(res["winner"] == -1)),
              "mean_game_steps": float(np.mean(res["game_steps"])), "passes": int(np.max(res["game_steps"]))})


if __name__ == "__main__":
    main()
