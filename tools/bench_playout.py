"""The playout player (scripted.PlayoutPolicy, catan_playout_actions) measured:
(1) strength: one PlayoutPolicy at its defaults against three builders over `--episodes` evaluation games with random seat orders
    (fair share 0.25), once per playout style, and on the same games and orders one trader and one builder in its place;
(2) time: milliseconds per catan_playout_actions call at the defaults for `--rows` rows (hipEvents around one call each, `--reps` calls
    after a warm-up; the roots are a mix of game ages reached by the trader), and the share of it spent inside catan_step - measured on
    a replica of the call's loop driven from Python (fork, sampler, hold as tensor operations, step) with events around every step;
    the replica's steps are the call's steps, its other parts are not, so the share is step time over the CALL's time.
Appends one JSON line per measurement, with the commit they were measured on, to `--out`.

With --parent-library (a libcatan_hip.so built from the parent commit) it first runs bench.py `--bench-pairs` times under each library,
alternating, every run a fresh process: with the player unused the change passes where its mean lies inside the spread (min..max) of the
parent's own runs, or above it.

usage: bench_playout.py [--episodes E] [--rows R [R ...]] [--reps K] [--skip-games] [--skip-calls] [--out FILE] [--commit TEXT]
                        [--parent-library libcatan_hip.so --bench-pairs B]"""
import argparse
import json
import os
import random
import sys

import parent_compare as pc


def games(args, emit, np):
    """(1) 512 games, one player in seat 0 against three builders"""
    from settlers_of_catan_rl_amd import evaluation as ev
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy, ScriptedPolicy, TraderPolicy
    n = args.episodes
    se = (0.25 * 0.75 / n) ** 0.5
    for name, make in (("playout_trader_style_vs_3_builders", lambda: PlayoutPolicy(playout_style="trader")),
                       ("playout_builder_style_vs_3_builders", lambda: PlayoutPolicy(playout_style="builder")),
                       ("trader_vs_3_builders", TraderPolicy), ("builder_vs_3_builders", ScriptedPolicy)):
        e = VecCatanEnv(n, seed=21, auto_reset=False)
        first, bot = make().rebind(e), ScriptedPolicy(e)
        res = ev.run_evaluation_episodes(e, [first, bot, bot, bot], ev.sample_orders(n, random.Random(3)), max_steps=args.max_steps)
        assert e.invalid_action_count() == 0
        w = res["winner"]
        rec = {"measurement": name, "episodes": n, "env_seed": 21, "orders_seed": 3, "max_steps": args.max_steps,
               "win_share_of_seat_0": float(np.mean(w == 0)), "fair_share": 0.25, "binomial_standard_error_at_fair_share": se,
               "draws": float(np.mean(w == -1)), "mean_game_steps": float(np.mean(res["game_steps"])),
               "mean_decisions_of_seat_0": float(np.mean(res["policy_decisions"]))}
        if isinstance(first, PlayoutPolicy):
            rec.update(candidates=list(first.candidates), playouts=first.playouts, depth=first.depth, determinise=first.determinise,
                       calls=first.step_idx, sim_games=first.sim.n, sim_invalid_actions=first.sim.invalid_action_count(),
                       sim_inconsistent_deals=first.sim.inconsistent_deal_count())
        emit(rec)


def call_times(args, emit, torch):
    """(2) ms per call and the share of catan_step"""
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy
    pol = PlayoutPolicy()
    C, K, D = sum(pol.candidates), pol.playouts, pol.depth
    mmm = lambda xs: [min(xs), sorted(xs)[len(xs) // 2], max(xs)]
    for rows in args.rows:
        root = VecCatanEnv(rows, seed=0)
        for _ in range(args.mix_steps):
            root.step(root.sample_scripted_actions(style="trader"))
        sim = VecCatanEnv(rows * C * K, seed=0, env_id0=1 << 40, auto_reset=False)
        kw = dict(candidates=pol.candidates, playouts=K, depth=D, playout_style=pol.playout_style, determinise=pol.determinise)
        idx = iter(range(3 + args.reps))             # three warm-up calls, then `reps` timed ones, events around each
        t = pc.event_call_times({"call": lambda: root.playout_actions(sim, step_idx=next(idx), **kw)}, 1, args.reps, warm=3)
        ms = [us / 1e3 for us in t["call"]["device_us"]]          # min, median, max
        # the replica: the same fork, the playout style in every seat from the first step on, finished games frozen
        src = torch.arange(rows, device=root.device).repeat_interleave(C * K)
        off = ((torch.arange(rows * C * K, device=root.device) % K) + 1) << 22
        step_ms = []
        for _ in range(max(2, args.reps // 2)):
            sim.fork_from(root, src, draw_offset=off)
            held = torch.zeros(rows * C * K, dtype=torch.bool, device=root.device)
            evs = []
            for d in range(D):
                a = sim.sample_scripted_actions(style=pol.playout_style)
                a[:, 0] = torch.where(held, torch.full_like(a[:, 0], -1), a[:, 0])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, done = sim.step(a)
                e1.record()
                held |= done.bool()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            step_ms.append(sum(x.elapsed_time(y) for x, y in evs))
        call, steps = ms[1], sorted(step_ms)[len(step_ms) // 2]
        emit({"measurement": "ms_per_call", "rows": rows, "candidates": list(pol.candidates), "playouts": K, "depth": D, "sims": rows * C * K,
              "playout_style": pol.playout_style, "determinise": pol.determinise, "reps": args.reps, "call_ms_min_median_max": ms,
              "replica_step_ms_sum_min_median_max": mmm(step_ms), "share_of_catan_step": steps / call,
              "us_per_sim_step": call * 1e3 / (rows * C * K * D)})
        assert root.invalid_action_count() == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-library")
    ap.add_argument("--bench-pairs", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=4096)
    ap.add_argument("--bench-warmup", type=int, default=256)
    ap.add_argument("--bench-child", action="store_true")
    ap.add_argument("--library")
    ap.add_argument("--episodes", type=int, default=512)
    ap.add_argument("--max-steps", type=int, default=2500)
    ap.add_argument("--rows", type=int, nargs="+", default=[128, 2048])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--mix-steps", type=int, default=300, help="untimed steps that spread the roots over the phases of play")
    ap.add_argument("--skip-games", action="store_true")
    ap.add_argument("--skip-calls", action="store_true")
    ap.add_argument("--out", type=str, default=os.path.join(pc.ROOT, "profiles", "playout_policy_bench.txt"))
    ap.add_argument("--commit", type=str, default=None, help="the commit of this tree (default: git rev-parse HEAD)")
    args = ap.parse_args()
    if args.bench_child:
        return pc.bench_py_child(args.library, args.bench_steps, args.bench_warmup)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "a")
    if args.parent_library:                 # first, while this process has not touched the device
        pc.bench_py_section(args, out, "player", __file__)
    import numpy as np
    import torch
    out.write("\nPlayout player (catan_playout_actions, scripted.PlayoutPolicy): measurements of tools/bench_playout.py\n"
              "commit: {}\ndevice: {}\ncommand: bench_playout.py {}\n"
              "One JSON line per measurement.  win_share_of_seat_0: the share of the games won by the player named first in `measurement`\n"
              "(seat orders drawn by evaluation.sample_orders).  ms_per_call: hipEvents around single calls through Python and ctypes.\n\n".format(
                  args.commit or pc.commit_of_tree(), torch.cuda.get_device_name(0), " ".join(a for i, a in enumerate(sys.argv[1:]) if a != "--commit" and sys.argv[i] != "--commit")))

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    if not args.skip_calls:
        call_times(args, emit, torch)
    if not args.skip_games:
        games(args, emit, np)


if __name__ == "__main__":
    main()
