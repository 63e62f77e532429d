#!/usr/bin/env python
"""Self-play PPO training on the batched HIP env - the loop of the reference's RL/robust_train.py with its defaults
(RL/ppo/arguments.py), one process per GPU (torch.distributed over RCCL when launched with torch.distributed.run).

    python tools/train.py --envs 65536 --updates 10 --league 8
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=640, help="games per GPU (reference: 128 processes x 5 envs)")
    ap.add_argument("--num-steps", type=int, default=200)
    ap.add_argument("--ppo-epoch", type=int, default=10)
    ap.add_argument("--num-mini-batch", type=int, default=64)
    ap.add_argument("--updates", type=int, default=2)
    ap.add_argument("--league", type=int, default=8, help="max distinct opponent snapshots in play (0: pure self-play)")
    ap.add_argument("--eval-every", type=int, default=25)
    ap.add_argument("--num-eval-episodes", type=int, default=128)
    ap.add_argument("--eval-max-steps", type=int, default=2500)
    ap.add_argument("--eval-scripted-baseline", action="store_true",
                    help="every evaluation also plays the rule-based player (scripted.ScriptedPolicy): log[\"scripted\"], comparable across runs")
    ap.add_argument("--eval-trader-baseline", action="store_true",
                    help="every evaluation also plays the trading rule-based player (scripted.TraderPolicy): log[\"trader\"]")
    ap.add_argument("--eval-playout-baseline", action="store_true",
                    help="every evaluation also plays the playout player (scripted.PlayoutPolicy, at its defaults): log[\"playout\"]")
    ap.add_argument("--eval-ladder", action="store_true",
                    help="every evaluation also plays the net against builder, trader and random in a tournament: log[\"ladder\"] = its rating with the builder at 0, "
                         "the standard error and the number of games")
    ap.add_argument("--checkpoint", type=str, default="")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--lstm", action="store_true", help="include_lstm (build_agent_model.py:26): LSTM policy + truncated BPTT")
    ap.add_argument("--diagnostics", action="store_true",
                    help="PPOConfig.diagnostics: every update's line carries \"ppo\" (per-epoch KL, clip fractions, explained variance, gradient norm)")
    ap.add_argument("--league-stats", action="store_true",
                    help="count on the device who won the finished games per opponent snapshot: every update's line carries \"league\"")
    ap.add_argument("--league-sampling", choices=["reference", "pfsp"], default="reference",
                    help="pfsp: draw the snapshots the central policy does badly against more often (implies --league-stats)")
    ap.add_argument("--start-pool", metavar="FILE", default="",
                    help="a start pool saved by start_pool.save (tools/make_start_pool.py): re-dealt games start from its positions; every update's line carries \"start_pool\"")
    ap.add_argument("--start-pool-fresh", metavar="P", type=float, default=0.0, help="the share of deals that stay fresh with --start-pool")
    ap.add_argument("--start-pool-outcomes", action="store_true",
                    help="with --start-pool: tally the finished games per pool entry on the device; every update's line carries them under \"start_pool\"")
    ap.add_argument("--start-pool-sampling", choices=["uniform", "balanced"], default="uniform",
                    help="balanced: draw the pool entries whose result is still open more often (implies --start-pool-outcomes)")
    ap.add_argument("--teacher", choices=["scripted", "trader", "playout"], default=None,
                    help="kickstarting: the rule-based player (trader: its trading style; playout: the playout player, whose rollouts are stepped lock-step) labels every decision of the rollouts; every update's line carries \"teacher\"")
    ap.add_argument("--playout-k", metavar="K", type=int, default=None, help="with --teacher playout: playouts per candidate (default: PlayoutPolicy's)")
    ap.add_argument("--playout-depth", metavar="D", type=int, default=None, help="with --teacher playout: env steps per playout")
    ap.add_argument("--playout-randoms", metavar="R", type=int, default=None, help="with --teacher playout: uniform-random candidates beside the builder's and the trader's")
    ap.add_argument("--teacher-coef", metavar="C", type=float, default=0.0, help="with --teacher: the imitation term's coefficient at update 0")
    ap.add_argument("--teacher-coef-updates", metavar="K", type=int, default=0,
                    help="the coefficient falls linearly to 0 over K updates (0: constant); after that the collector stops labelling")
    ap.add_argument("--teacher-only-updates", metavar="J", type=int, default=0, help="the first J updates are pure imitation (no policy-gradient, no entropy term)")
    args = ap.parse_args()
    league_stats = args.league > 0 and (args.league_stats or args.league_sampling == "pfsp")
    import torch
    from settlers_of_catan_rl_amd import dist as cdist
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    rank, local_rank, world = cdist.init_from_env()
    from settlers_of_catan_rl_amd.env import VecCatanEnv
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    from settlers_of_catan_rl_amd.rollout import RolloutCollector
    from settlers_of_catan_rl_amd.train import PPOTrainer, PPOConfig
    from settlers_of_catan_rl_amd.league import League
    from settlers_of_catan_rl_amd import evaluation, train_loop
    torch.manual_seed(args.seed)
    env_id0, n = cdist.shard(rank, args.envs)
    env = VecCatanEnv(n, seed=args.seed, env_id0=env_id0)          # game_manager.py:16: EnvWrapper() defaults (sparse win reward)
    net = CatanPolicy(include_lstm=args.lstm).cuda()
    cdist.broadcast_parameters(net)
    teach = dict(teacher=args.teacher, teacher_coef=args.teacher_coef, teacher_coef_updates=args.teacher_coef_updates,
                 teacher_only_updates=args.teacher_only_updates) if args.teacher else {}
    if args.teacher == "playout":
        teach.update(playout_k=args.playout_k, playout_depth=args.playout_depth, playout_randoms=args.playout_randoms)
    teacher = train_loop.make_teacher(train_loop.TrainArgs(**teach), env)
    col = RolloutCollector(env, net, args.num_steps, seed=rank, autocast_dtype=torch.bfloat16, **(dict(league_stats=True) if league_stats else {}),
                           **(dict(teacher=teacher) if teacher is not None else {}))
    tr = PPOTrainer(net, PPOConfig(ppo_epoch=args.ppo_epoch, num_mini_batch=args.num_mini_batch, diagnostics=args.diagnostics), seed=rank)
    random_net = CatanPolicy(include_lstm=args.lstm).cuda().eval()                                   # robust_train.py:76-78: the evaluation opponent

    def evaluate(policy, update_num):
        log, summary = evaluation.run_evaluation_protocol(lambda m: VecCatanEnv(m, seed=args.seed + 1000 + update_num, env_id0=1 << 40, auto_reset=False),
                                                          policy, random_net, args.num_eval_episodes, update_num,
                                                          max_steps=args.eval_max_steps, autocast_dtype=torch.bfloat16,
                                                          baselines=train_loop.eval_baselines(targs))
        ladder = train_loop.eval_ladder(targs)
        if ladder is not None:
            log["ladder"] = ladder(policy, VecCatanEnv(args.num_eval_episodes, seed=args.seed + 1000 + update_num, env_id0=1 << 41),
                                   max_steps=args.eval_max_steps, autocast_dtype=torch.bfloat16)
            summary += "Ladder (builder = 0): rating {rating:.1f} +/- {stderr:.1f} over {games} games. \n\n".format(**log["ladder"])
        return log, summary

    lg = League(max_distinct=args.league, seed=rank, sampling=args.league_sampling) if args.league > 0 else None
    targs = train_loop.TrainArgs(num_steps=args.num_steps, eval_every=args.eval_every, num_eval_episodes=args.num_eval_episodes,
                                 eval_scripted_baseline=args.eval_scripted_baseline, eval_trader_baseline=args.eval_trader_baseline,
                                 eval_playout_baseline=args.eval_playout_baseline, eval_ladder=args.eval_ladder, **teach,
                                 **(dict(start_pool=args.start_pool, start_pool_fresh=args.start_pool_fresh, start_pool_outcomes=args.start_pool_outcomes,
                                        start_pool_sampling=args.start_pool_sampling) if args.start_pool else {}))
    loop = train_loop.TrainingLoop(env, net, col, tr, targs, league=lg, make_net=lambda: CatanPolicy(include_lstm=args.lstm).cuda(),
                                   evaluate=evaluate if rank == 0 else None, checkpoint_path=args.checkpoint or None)
    for _ in range(args.updates):
        out = loop.run_update()
        if rank == 0:
            if out["eval"]:
                print(out["eval"])
            if "ppo" in out:
                fmt = lambda xs: " ".join("%.3e" % x for x in xs)
                for k in ("approx_kl", "clip_fraction", "explained_variance"):
                    print(f"update {out['update']} {k:18s} per epoch: {fmt(out['ppo'][k])}", flush=True)
            if "league" in out:
                lo, hi = (f(range(len(out["league"]["serials"])), key=lambda i: out["league"]["central_share"][i]) for f in (min, max))
                print("update %d central share: lowest %.3f against snapshot %d, highest %.3f against snapshot %d (%d snapshots, %d games tallied)"
                      % (out["update"], out["league"]["central_share"][lo], out["league"]["serials"][lo], out["league"]["central_share"][hi],
                         out["league"]["serials"][hi], len(out["league"]["serials"]), out["league"]["totals"]["games_tallied"]), flush=True)
            print(json.dumps({k: v for k, v in out.items() if k != "eval"}), flush=True)
    cdist.finalize()


if __name__ == "__main__":
    main()
