"""What the tournament costs and what its streaming loop buys, measured, with one ladder of the fixed players.

  off      bench.py with the parent commit's library and this commit's in alternating fresh-process pairs: the tournament is never enabled
           there, and the change passes by parent_compare.verdict
  on       catan_step and catan_step_deferred in microseconds per call at 65 536 games with the tournament off, with 5 lineups (the LDS
           table) and with 65 536 (global atomics), a fresh process per run, the three rotating inside a round
  runner   games per second of tournament.run_tournament (n game slots x E episodes, streaming) against evaluation.run_evaluation_episodes
           called E times on n games (each batch waits for its longest game): the same players, the same lineups and seats - the seat
           rule's - and the same n x E games, alternating in one process
  ladder   builder, trader, random and the playout player over all_lineups(4): shares, ratings and standard errors as measured

usage: bench_tournament.py [--parent-library libcatan_hip.so] [--bench-pairs B] [--games N] [--calls K] [--warmup W] [--runs R]
                           [--runner-envs N] [--runner-episodes E] [--runner-rounds R] [--ladder-envs N] [--ladder-episodes E]
                           [--out profiles/tournament_bench.txt]"""
import argparse
import json
import os
import time

import parent_compare as pc

FIXED = ("builder", "trader", "random")


def _players(names):
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy, RandomPolicy, ScriptedPolicy, TraderPolicy
    make = {"builder": ScriptedPolicy, "trader": TraderPolicy, "random": RandomPolicy, "playout": PlayoutPolicy}
    return [make[k]() for k in names]


def step_child(a):
    pc.use_library(a.library)
    from settlers_of_catan_rl_amd import tournament
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    env = VecCatanEnv(a.games, seed=1)
    out = {"mode": a.mode}
    if a.mode != "off":
        import numpy as np
        L = int(a.mode)
        lineups = tournament.all_lineups(3)[:L] if L <= 15 else np.random.RandomState(1).randint(0, 8, size=(L, 4))
        env.enable_tournament(lineups, 8, 0)
        env.reset()

    def between(name, phase):                       # the games booked in the timed calls alone
        t = env.tournament_table(reset=True)
        if phase == "timed":
            out[name + "_seen"] = int(t[-1, 0])
    out.update(pc.step_call_times(env, a.calls, a.warmup, between if a.mode != "off" else None))
    print("RESULT " + json.dumps(out), flush=True)


def _schedule(n, E, lineups, e):
    """episode e of every game slot as run_evaluation_episodes takes it: (assignment [n, 4], orders [n, 4]) by the seat rule"""
    import numpy as np
    from settlers_of_catan_rl_amd import tournament
    assignment, orders = np.zeros((n, 4), dtype=np.int64), np.zeros((n, 4), dtype=np.int64)
    for g in range(n):
        lineup, perm = tournament.seating(tournament.episode_index(g, e, E), len(lineups))
        assignment[g] = lineups[lineup]                      # policy i of the game is the player at lineup position i
        for p in range(4):
            orders[g, perm[p]] = p + 1                       # ... and plays the PlayerId whose position it holds
    return assignment, orders


def runner_child(a):
    import torch
    from settlers_of_catan_rl_amd import evaluation, tournament
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    n, E = a.runner_envs, a.runner_episodes
    lineups = tournament.all_lineups(len(FIXED))
    rows = []
    for r in range(a.runner_rounds):
        for how in pc.order(["streaming", "batches"], r, "alternate"):
            players = _players(FIXED)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if how == "streaming":
                res = tournament.run_tournament(VecCatanEnv(n, seed=10 + r), players, lineups, E, max_steps=a.max_steps)
                games, draws, passes = int(res["table"][-1, 0]), int(res["table"][-1, 2]), res["passes"]
            else:
                games = draws = passes = 0
                for e in range(E):
                    env = VecCatanEnv(n, seed=10 + r, env_id0=e << 32, auto_reset=False)
                    for p in players:
                        p.rebind(env)
                    assignment, orders = _schedule(n, E, lineups, e)
                    out = evaluation.run_evaluation_episodes(env, players, orders, max_steps=a.max_steps, assignment=assignment)
                    games += n
                    draws += int((out["winner"] < 0).sum())
                    passes += int(out["game_steps"].max())
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rows.append({"round": r, "how": how, "games": games, "draws": draws, "passes": passes, "seconds": dt, "games_per_s": games / dt})
            print(json.dumps(rows[-1]), flush=True)
    print("RESULT " + json.dumps({"rows": rows}), flush=True)


def ladder_child(a):
    from settlers_of_catan_rl_amd import tournament
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    names = list(FIXED) + ["playout"]
    lineups = tournament.all_lineups(len(names))
    t0 = time.perf_counter()
    res = tournament.run_tournament(VecCatanEnv(a.ladder_envs, seed=20), _players(names), lineups, a.ladder_episodes, max_steps=a.max_steps)
    dt = time.perf_counter() - t0
    fit = tournament.fit_ratings(res["table"], lineups, len(names), anchor=0)
    text = tournament.report(res, names=names, ratings=fit)
    print("RESULT " + json.dumps({"text": text, "seconds": dt, "passes": res["passes"], "totals": [int(x) for x in res["table"][-1, :6]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-library")
    ap.add_argument("--bench-pairs", type=int, default=5, help="pairs of bench.py runs (0: none)")
    ap.add_argument("--bench-steps", type=int, default=4096)
    ap.add_argument("--bench-warmup", type=int, default=256)
    ap.add_argument("--games", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--runner-envs", type=int, default=1024)
    ap.add_argument("--runner-episodes", type=int, default=4)
    ap.add_argument("--runner-rounds", type=int, default=3)
    ap.add_argument("--ladder-envs", type=int, default=256)
    ap.add_argument("--ladder-episodes", type=int, default=4)
    ap.add_argument("--max-steps", type=int, default=2500)
    ap.add_argument("--out", default=os.path.join(pc.ROOT, "profiles", "tournament_bench.txt"))
    ap.add_argument("--child", choices=["step", "runner", "ladder"])
    ap.add_argument("--bench-child", action="store_true")
    ap.add_argument("--mode", default="off")
    ap.add_argument("--library")
    a = ap.parse_args()
    if a.bench_child:
        return pc.bench_py_child(a.library, a.bench_steps, a.bench_warmup)
    if a.child:
        return {"step": step_child, "runner": runner_child, "ladder": ladder_child}[a.child](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as out:
        out.write(f"The tournament (DESIGN.md 8.16), measured by tools/bench_tournament.py on one MI355X; commit {pc.commit_of_tree()}\n")
        if a.bench_pairs and a.parent_library:
            pc.bench_py_section(a, out, "tournament", __file__)
        modes = ["off", "5", "65536"]
        rows = {m: [] for m in modes}
        for r in range(a.runs):
            for m in pc.order(modes, r, "rotate"):
                rows[m].append(pc.run_child(__file__, ["--child", "step", "--games", str(a.games), "--calls", str(a.calls), "--warmup", str(a.warmup),
                                                      "--mode", m], 300, "RESULT "))
                print(f"run {r} lineups {m:6s} {json.dumps(rows[m][-1])}", flush=True)
        lines = ["", f"catan_step and catan_step_deferred, microseconds per call: {a.games} games, {a.calls} timed calls behind {a.warmup}, {a.runs} runs each, a fresh",
                 "process per run, the three configurations rotating; a call = catan_sample_random_actions + the step (the random policy knows of no",
                 "retirement: E = 0)"]
        for key in ("catan_step_us", "catan_step_deferred_us"):
            lines.append(key[:-3])
            for m in modes:
                v = [x[key] for x in rows[m]]
                seen = "" if m == "off" else f"   games booked in a run's timed calls {rows[m][0][key[:-3] + '_seen']}"
                lines.append(f"  {'off' if m == 'off' else m + ' lineups':14s} runs {' '.join(f'{x:8.2f}' for x in v)}   mean {sum(v) / len(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}{seen}")
            for m in modes[1:]:
                lines.append(f"  {m} lineups against off: " + pc.sentence([x[key] for x in rows[m]], [x[key] for x in rows["off"]], False))
        text = "\n".join(lines) + "\n"
        print(text, flush=True)
        out.write(text)
        out.flush()
        common = ["--max-steps", str(a.max_steps)]
        res = pc.run_child(__file__, ["--child", "runner", "--runner-envs", str(a.runner_envs), "--runner-episodes", str(a.runner_episodes),
                                      "--runner-rounds", str(a.runner_rounds)] + common, 1500, "RESULT ")
        gps = {how: [x["games_per_s"] for x in res["rows"] if x["how"] == how] for how in ("streaming", "batches")}
        lines = ["", f"The runner: builder, trader and random over all_lineups(3) (15 lineups), {a.runner_envs} game slots x {a.runner_episodes} episodes, draw cap {a.max_steps};",
                 f"run_tournament (streaming) against run_evaluation_episodes called {a.runner_episodes} times on {a.runner_envs} games without auto-reset (batches), the same lineups",
                 "and seats, alternating in one process; host clock around each, device synchronised"]
        lines += ["  round {round} {how:10s} games {games} draws {draws} passes {passes} seconds {seconds:.2f} games/s {games_per_s:.1f}".format(**x) for x in res["rows"]]
        mean = lambda v: sum(v) / len(v)
        lines.append(f"  games/s: streaming mean {mean(gps['streaming']):.1f} (min {min(gps['streaming']):.1f}, max {max(gps['streaming']):.1f}); batches mean "
                     f"{mean(gps['batches']):.1f} (min {min(gps['batches']):.1f}, max {max(gps['batches']):.1f}); ratio of the means {mean(gps['streaming']) / mean(gps['batches']):.3f}")
        text = "\n".join(lines) + "\n"
        print(text, flush=True)
        out.write(text)
        out.flush()
        res = pc.run_child(__file__, ["--child", "ladder", "--ladder-envs", str(a.ladder_envs), "--ladder-episodes", str(a.ladder_episodes)] + common, 1500, "RESULT ")
        text = (f"\nOne ladder: builder, trader, random and the playout player (its defaults), all_lineups(4) = the one lineup of all four, {a.ladder_envs} game slots x\n"
                f"{a.ladder_episodes} episodes, draw cap {a.max_steps}: {res['passes']} passes in {res['seconds']:.1f} s; totals (seen, tallied, draws, unseated, seated, retired) {res['totals']}\n"
                + res["text"] + "\n")
        print(text, flush=True)
        out.write(text)


if __name__ == "__main__":
    main()
