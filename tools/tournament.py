#!/usr/bin/env python
"""A round-robin tournament between checkpoints and the fixed players, and their ratings on one scale.

    python tools/tournament.py builder trader random ckpt:run/update_200.pt ckpt:run/update_400.pt --out ratings.json

players: `builder`, `trader`, `random`, `playout` (scripted.ScriptedPolicy, TraderPolicy, RandomPolicy, PlayoutPolicy at its defaults) and
`ckpt:PATH` (a TrainingLoop.save file, the reference's checkpoint tuple or a bare state dict).  The first player is the rating scale's
zero.  --lineups all: every four of them (fewer than four players: every multiset of four); vs-anchors: every ckpt: player against three
copies of each fixed player and against the first three fixed players together."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXED = ("builder", "trader", "random", "playout")


def load_policy(path):
    import torch
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck["central_policy"] if isinstance(ck, dict) and "central_policy" in ck else (ck[0] if isinstance(ck, (tuple, list)) else ck)
    net = CatanPolicy(include_lstm=any(k.startswith("lstm") for k in sd))
    own = net.state_dict()
    net.load_state_dict({k: v for k, v in sd.items() if k in own})
    return net.cuda().eval()


def make_player(name):
    from settlers_of_catan_rl_amd.scripted import PlayoutPolicy, RandomPolicy, ScriptedPolicy, TraderPolicy
    if name.startswith("ckpt:"):
        return load_policy(name[5:])
    if name not in FIXED:
        raise SystemExit(f"unknown player {name!r}: one of {', '.join(FIXED)} or ckpt:PATH")
    return {"builder": ScriptedPolicy, "trader": TraderPolicy, "random": RandomPolicy, "playout": PlayoutPolicy}[name]()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("players", nargs="+", help="builder | trader | random | playout | ckpt:PATH")
    ap.add_argument("--lineups", choices=["all", "vs-anchors"], default="all")
    ap.add_argument("--episodes-per-game", type=int, default=4)
    ap.add_argument("--envs", type=int, default=1024, help="game slots played at once")
    ap.add_argument("--max-steps", type=int, default=2500, help="env steps after which a game is reset and booked as a draw")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="", help="ratings.json: the table, the per-player summary and the ratings")
    a = ap.parse_args()
    import torch
    from settlers_of_catan_rl_amd import tournament
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    names = list(a.players)
    if a.lineups == "all":
        lineups = tournament.all_lineups(len(names))
    else:
        candidates = [i for i, x in enumerate(names) if x.startswith("ckpt:")]
        anchors = [i for i, x in enumerate(names) if not x.startswith("ckpt:")]
        if not candidates or not anchors:
            raise SystemExit("--lineups vs-anchors needs at least one ckpt: player and one fixed player")
        lineups = tournament.versus_anchors(candidates, anchors)
    torch.manual_seed(a.seed)
    players = [make_player(x) for x in names]
    env = VecCatanEnv(a.envs, seed=a.seed)
    res = tournament.run_tournament(env, players, lineups, a.episodes_per_game, max_steps=a.max_steps, autocast_dtype=torch.bfloat16)
    fit = tournament.fit_ratings(res["table"], lineups, len(names), anchor=0)
    print(tournament.report(res, names=names, ratings=fit))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"players": names, "lineups": lineups.tolist(), "episodes_per_game": a.episodes_per_game, "envs": a.envs, "seed": a.seed,
                       "max_steps": a.max_steps, "table": res["table"].tolist(), "summary": res["players"], "passes": res["passes"],
                       "ratings": {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in fit.items()}}, f, indent=1)


if __name__ == "__main__":
    main()
