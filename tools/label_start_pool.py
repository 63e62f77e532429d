"""Labels the positions of a start pool by playouts (settlers_of_catan_rl_amd/start_pool.py): who wins the games that
begin at each entry.

usage: label_start_pool.py POOL.npz --games N --steps S [--player scripted|random] [--seed K] -o OUT.npz

Builds an env of N games with auto_reset, installs the pool with every deal taken from it (fresh_share = 0), switches the per-entry outcome
tallies on and plays S lock-step steps with the rule-based player (scripted.ScriptedPolicy's sampler) or the library's uniform-random
policy in every seat.  Writes the pool back with the tallies attached (StartPool.outcomes) and prints one summary line: entries played,
games tallied, and the share of the played entries in which one seat took at least 90 % of the games."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DECIDED_PERCENT = 90


def summary_line(table):
    """table: [m + 1, 8] outcome tallies (spec.START_POOL_OUTCOME_FIELDS), the last row the fresh deals'"""
    import numpy as np
    t = np.asarray(table).astype(np.int64)[:-1]
    games, wins = t[:, 0], t[:, 1:5]
    played = games > 0
    decided = played & (wins.max(axis=1) * 100 >= DECIDED_PERCENT * games)
    share = float(decided.sum()) / float(played.sum()) if played.any() else float("nan")
    return (f"{int(played.sum())} of {len(t)} entries played, {int(games.sum())} games tallied, "
            f"{100.0 * share:.1f} % of the played entries have one seat with at least {DECIDED_PERCENT} % of the games")


def main(argv=None, make_env=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("pool", help="a pool saved by start_pool.save (tools/make_start_pool.py)")
    ap.add_argument("--games", type=int, required=True)
    ap.add_argument("--steps", type=int, required=True)
    ap.add_argument("--player", choices=["scripted", "random"], default="scripted")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("-o", "--out", required=True)
    a = ap.parse_args(argv)
    from settlers_of_catan_rl_amd import start_pool
    pool = start_pool.load(a.pool)
    if make_env is None:
        from settlers_of_catan_rl_amd.env import VecCatanEnv
        make_env = lambda n, seed: VecCatanEnv(n, seed=seed, auto_reset=True)
    env = make_env(a.games, a.seed)
    env.set_start_pool(pool.blobs, fresh_share=0.0)
    env.enable_start_pool_outcomes()
    env.reset()
    if a.player == "random":
        env.random_rollout(0, a.steps)          # (lock-step: the deferred random rollout is refused under a pool)
    else:
        for _ in range(a.steps):
            env.step(env.sample_scripted_actions())
    out = env.start_pool_outcomes()
    pool.add_outcomes(out)
    start_pool.save(pool, a.out)
    print(f"{a.out}: {summary_line(out['table'])}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
