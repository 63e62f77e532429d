"""evaluation/run_forward_search_evaluation.py of the reference, on the device: seat 0 of every game is the forward-search
planner, the other three seats are plain nets; all --num-games games run at once.  Prints the fraction of games the planner won
and saves (winners, game steps, victory points, planner decisions, sorted action-type counts) to forward_policy_evaluation.pt.

Checkpoints are read from --results-dir (default RL/results, as the reference does relative to the working directory).
--num-subprocesses is accepted and ignored (there are no worker processes); --sims-per-root replaces the wall-clock budget of
--max-thinking-time with a fixed number of simulations per decision."""
import argparse
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--base-policy-file", type=str, required=True)
    p.add_argument("--max-thinking-time", type=float, default=10.0)
    p.add_argument("--gamma", type=float, default=0.999)
    p.add_argument("--num-subprocesses", type=int, default=32)
    p.add_argument("--num-games", type=int, default=100)
    p.add_argument("--max-init-actions", type=int, default=10)
    p.add_argument("--max-depth", type=int, default=15)
    p.add_argument("--consider-all-moves-for-opening-placements", action="store_true", default=False)
    p.add_argument("--dont-propose-devcards", action="store_true", default=False)
    p.add_argument("--dont-propose-trades", action="store_true", default=False)
    p.add_argument("--zero-opponent-hidden-states", action="store_true", default=False)
    p.add_argument("--other-policies", type=str, default="")
    p.add_argument("--sims-per-root", type=int, default=None)
    p.add_argument("--sims-per-round", type=int, default=16)
    p.add_argument("--results-dir", type=str, default=os.path.join("RL", "results"))
    args = p.parse_args(argv)
    torch.manual_seed(10); np.random.seed(10); random.seed(10)
    from settlers_of_catan_rl_amd import evaluation, reference_api as ra
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    load = lambda name: torch.load(os.path.join(args.results_dir, name), map_location="cpu")  # noqa: E731
    sd = load(args.base_policy_file)
    if args.other_policies != "":
        names = args.other_policies.split(" ")
        names = names * 3 if len(names) == 1 else names
        others_sd = [load(names[i]) for i in range(3)]
    else:
        others_sd = [sd, sd, sd]
    planner = ra.ForwardSearchPolicy(sd, None, args.max_init_actions, args.max_depth, args.max_thinking_time, gamma=args.gamma,
                                     num_subprocesses=args.num_subprocesses, zero_opponent_hidden_states=args.zero_opponent_hidden_states,
                                     consider_all_moves_for_opening_placement=args.consider_all_moves_for_opening_placements,
                                     dont_propose_trades=args.dont_propose_trades, dont_propose_devcards=args.dont_propose_devcards,
                                     sims_per_root=args.sims_per_root, sims_per_round=args.sims_per_round)
    others = []
    for o in others_sd:
        net = CatanPolicy().to(planner._device).eval()
        net.load_reference_state_dict(o)
        others.append(net)
    return evaluation.run_forward_search_evaluation(planner, others, args.num_games)


if __name__ == "__main__":
    main()
