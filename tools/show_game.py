"""Prints a recorded game, one line per action (settlers_of_catan_rl_amd/record.py describe), or records evaluation games.

usage: show_game.py RECORD.npz
       show_game.py --from-eval CHECKPOINT --games K --out DIR [--seed S] [--max-steps M]

--from-eval: plays K evaluation games of the checkpoint's policy (policy 0; a TrainingLoop.save file, the reference's checkpoint tuple
or a bare state dict; the word `scripted` instead of a file: the rule-based player itself) against three rule-based players and saves
their records as DIR/game_<id>.npz.  Needs the GPU, as every replay does."""
import argparse
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _load_policy(path):
    import torch
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck["central_policy"] if isinstance(ck, dict) and "central_policy" in ck else (ck[0] if isinstance(ck, (tuple, list)) else ck)
    net = CatanPolicy()
    own = net.state_dict()
    net.load_state_dict({k: v for k, v in sd.items() if k in own})
    return net.cuda().eval()


def from_eval(checkpoint, games, out_dir, seed=10, max_steps=2500):
    from settlers_of_catan_rl_amd import evaluation, record
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.scripted import ScriptedPolicy
    env = VecCatanEnv(games, seed=seed, auto_reset=False)
    bot = ScriptedPolicy(env)
    central = bot if checkpoint == "scripted" else _load_policy(checkpoint)
    res = evaluation.run_evaluation_episodes(env, [central, bot, bot, bot], evaluation.sample_orders(games, random.Random(seed)),
                                             max_steps=max_steps, record=games)
    os.makedirs(out_dir, exist_ok=True)
    paths = []
    for rec, winner in zip(res["records"], res["winner"]):
        paths.append(os.path.join(out_dir, f"game_{rec.game_id}.npz"))
        record.save(rec, paths[-1])
        print(f"{paths[-1]}: {rec.length} actions, " + ("a draw" if winner < 0 else f"won by policy {int(winner)}"))
    return paths


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("record", nargs="?", help="a record saved by record.save")
    ap.add_argument("--from-eval", metavar="CHECKPOINT")
    ap.add_argument("--games", type=int, default=4)
    ap.add_argument("--out", metavar="DIR")
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--max-steps", type=int, default=2500)
    a = ap.parse_args(argv)
    if a.from_eval:
        if not a.out:
            ap.error("--from-eval needs --out DIR")
        from_eval(a.from_eval, a.games, a.out, a.seed, a.max_steps)
        return 0
    if not a.record:
        ap.error("a record file, or --from-eval")
    from settlers_of_catan_rl_amd import record
    print("\n".join(record.describe(record.load(a.record))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
