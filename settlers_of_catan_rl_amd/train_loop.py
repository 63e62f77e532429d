"""The training loop around the PPO update (reference RL/robust_train.py:50-176 `run_update`), on one batched env per GPU.

Per update: linear learning-rate decay (RL/ppo/utils.py:1-5) -> rollout collection (rollout.RolloutCollector) -> PPO update
(train.PPOTrainer) -> entropy-coefficient annealing (robust_train.py:108-117) and dense-reward annealing (:119-124) ->
league bookkeeping (snapshot every `add_policy_every` updates, opponents re-drawn every `update_opponent_policies_every`,
:135-141) -> evaluation protocol every `eval_every` updates (:143-151) -> checkpoint.  The reference's watchdog /
fail_handler (:160-176) restarts crashed worker processes; there are none here.  The checkpoint holds the same items as the
reference's tuple (central state-dict, league deque, eval logs, update number, args) in a dict.
"""
import copy
import time

import torch

from . import dist as cdist
from . import spec


class TrainArgs(object):
    """RL/ppo/arguments.py defaults (only the fields this loop reads)."""
    lr = 3e-4
    use_linear_lr_decay = True
    entropy_coef_start = 0.04
    entropy_coef_final = 0.005
    entropy_coef_start_anneal = 500
    entropy_coef_end_anneal = 1500
    dense_reward_anneal_start = -1
    dense_reward_anneal_end = -1
    num_steps = 200
    total_env_steps = int(1e9)
    add_policy_every = 4
    update_opponent_policies_every = 1
    eval_every = 25
    num_eval_episodes = 128
    start_pool = None                    # opt-in: a start_pool.StartPool, blobs [m, 736] or the path of a saved pool - re-dealt games start from its positions
    start_pool_fresh = 0.0               # ... except for this share of the deals, which stay fresh
    start_pool_outcomes = False          # opt-in: the finished games are tallied per pool entry on the device -> log["start_pool"]["outcomes"]
    start_pool_sampling = "uniform"      # "balanced": the entries whose result is still open are drawn more often (implies the outcomes)
    eval_scripted_baseline = False       # opt-in: the evaluation also plays the rule-based player (scripted.ScriptedPolicy) -> log["scripted"]
    eval_trader_baseline = False         # opt-in: ... and the trading rule-based player (scripted.TraderPolicy) -> log["trader"]
    eval_playout_baseline = False        # opt-in: ... and the playout player (scripted.PlayoutPolicy) -> log["playout"]
    eval_ladder = False                  # opt-in: ... and a tournament of the net against builder, trader and random -> log["ladder"]
    eval_ladder_episodes = 2             # ... episodes per game slot in it
    teacher = None                       # opt-in kickstarting: "scripted" - the rule-based player labels the rollouts (make_teacher); "trader": its trading style (8.14); "playout": the playout player (8.15)
    playout_k = None                     # ... teacher "playout": PlayoutPolicy's playouts, depth and randoms (None: its defaults)
    playout_depth = None
    playout_randoms = None
    teacher_coef = 0.0                   # ... the imitation term's coefficient at update 0
    teacher_coef_updates = 0             # ... falling linearly to 0 over this many updates (0: constant); at 0 the collector stops labelling
    teacher_only_updates = 0             # ... the first J updates are pure imitation (PPOConfig.teacher_only)

    def __init__(self, **kw):
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


def eval_baselines(args):
    """The fixed opponents `args` adds to the evaluation protocol, as evaluation.run_evaluation_protocol(baselines=...) takes them;
    None (the default): the reference's protocol alone."""
    from .scripted import PlayoutPolicy, ScriptedPolicy, TraderPolicy
    out = {}
    if getattr(args, "eval_scripted_baseline", False):
        out["scripted"] = ScriptedPolicy
    if getattr(args, "eval_trader_baseline", False):
        out["trader"] = TraderPolicy
    if getattr(args, "eval_playout_baseline", False):
        out["playout"] = PlayoutPolicy
    return out or None


LADDER_ANCHORS = ("builder", "trader", "random")


def eval_ladder(args):
    """The rating ladder `args` adds to every evaluation; None (the default): none.  -> ladder(policy, env, **kw): plays `policy` against
    the rule-based builder, the trader and the uniform-random sampler on `env` (games with auto_reset, freshly made) by
    tournament.versus_anchors - the net against three copies of each and against the three together,
    args.eval_ladder_episodes episodes per game slot; kw goes to tournament.run_tournament - and returns the log entry: the net's
    rating on the scale where the builder is 0 (tournament.fit_ratings, its default prior), the rating's standard error and the number
    of decided games behind both."""
    if not getattr(args, "eval_ladder", False):
        return None
    episodes = int(getattr(args, "eval_ladder_episodes", TrainArgs.eval_ladder_episodes))

    def ladder(policy, env, **kw):
        from . import tournament
        from .scripted import RandomPolicy, ScriptedPolicy, TraderPolicy
        players = [ScriptedPolicy(), TraderPolicy(), RandomPolicy(), policy]
        lineups = tournament.versus_anchors([3], [0, 1, 2])
        res = tournament.run_tournament(env, players, lineups, episodes, **kw)
        fit = tournament.fit_ratings(res["table"], lineups, len(players), anchor=0)
        return {"rating": float(fit["rating"][3]), "stderr": float(fit["stderr"][3]), "games": int(fit["games"])}
    return ladder


def make_teacher(args, env):
    """The teacher `args` asks for, as RolloutCollector(teacher=...) takes it; None (the default): no teacher, no call."""
    name = getattr(args, "teacher", None)
    if name is None or not getattr(args, "teacher_coef", 0.0) > 0:
        return None
    if name not in ("scripted", "trader", "playout"):
        raise ValueError(f"teacher must be 'scripted', 'trader', 'playout' or None, got {name!r}")
    from .scripted import PlayoutPolicy, ScriptedPolicy, TraderPolicy
    if name == "playout":
        opts = {k: getattr(args, a) for k, a in (("playouts", "playout_k"), ("depth", "playout_depth"), ("randoms", "playout_randoms"))
                if getattr(args, a, None) is not None}
        return PlayoutPolicy(env, **opts)
    return TraderPolicy(env) if name == "trader" else ScriptedPolicy(env)


def teacher_coef_at(update_num, args):
    """The imitation coefficient of update `update_num`: args.teacher_coef, falling linearly to 0 at update args.teacher_coef_updates
    (0 updates: constant).  0 without a teacher."""
    if getattr(args, "teacher", None) is None or not args.teacher_coef > 0:
        return 0.0
    k = int(args.teacher_coef_updates)
    if k <= 0:
        return float(args.teacher_coef)
    return float(args.teacher_coef) * max(0.0, 1.0 - update_num / float(k))


def linear_lr(update_num, num_updates, initial_lr):
    """RL/ppo/utils.py:1-5"""
    return initial_lr - (initial_lr * (update_num / float(num_updates)))


def entropy_coef_at(update_num, args, current):
    """robust_train.py:108-117: linear between the anneal bounds, untouched outside (update_num > start and <= end)."""
    if args.entropy_coef_start_anneal < update_num <= args.entropy_coef_end_anneal:
        s, e = args.entropy_coef_start_anneal, args.entropy_coef_end_anneal
        return args.entropy_coef_start + ((update_num - s) / (e - s)) * (args.entropy_coef_final - args.entropy_coef_start)
    return current


def reward_weight_at(update_num, args, current):
    """robust_train.py:119-124: dense-reward annealing factor 1 -> 0 between its bounds."""
    if args.dense_reward_anneal_start < update_num <= args.dense_reward_anneal_end:
        s, e = args.dense_reward_anneal_start, args.dense_reward_anneal_end
        return 1.0 + ((update_num - s) / (e - s)) * (0.0 - 1.0)
    return current


class TrainingLoop(object):
    def __init__(self, env, policy, collector, trainer, args=None, league=None, make_net=None, evaluate=None, checkpoint_path=None):
        """evaluate(policy, update_num) -> (log, summary) (evaluation.run_evaluation_protocol bound to an env factory and an
        opponent) or None; make_net() builds an empty net for league opponents."""
        self.env, self.policy, self.collector, self.trainer = env, policy, collector, trainer
        self.args = args or TrainArgs()
        self.league, self.make_net, self.evaluate = league, make_net, evaluate
        self.checkpoint_path = checkpoint_path
        world = torch.distributed.get_world_size() if torch.distributed.is_initialized() else 1
        self.steps_per_update = int(self.args.num_steps * env.n * world)                   # robust_train.py:93
        self.num_updates = int(self.args.total_env_steps) // self.steps_per_update          # :92
        self.update_num = 0
        self.entropy_coef = self.args.entropy_coef_start
        self.reward_weight = 1.0
        self.eval_logs = []
        self.start_time = time.time()
        trainer.cfg.entropy_coef = self.entropy_coef
        if self.args.start_pool is not None:
            # the pool on the env (unless the collector was built with one), then ONE reset: the first rollout's games already come from
            # the pool at the configured share; the collector's per-game bookkeeping starts over with them
            if not getattr(collector, "start_pool_on", False):
                collector.install_start_pool(self.args.start_pool, self.args.start_pool_fresh, self.args.start_pool_outcomes, self.args.start_pool_sampling)
            env.reset()
            env.start_pool_counts(reset=True)           # (the counts of a rollout are those of its own deals)
            collector.reset()
        if league is not None:
            if len(league.earlier) == 0:
                # a fresh start (robust_train.py:60-64): the deque gets the initial policy, and the FIRST rollout is played against
                # independently random-initialised opponents - the nets every reference worker builds for its policy slots 1..3
                # (game_manager.py:14); snapshots are drawn for the first time after update 0 (:140-141).  One such set serves all
                # games here (the reference has one per worker process).
                league.add(policy)
                nets = [make_net() for _ in range(3)]
                for nt in nets:
                    nt.eval()
                collector.set_opponents(nets, torch.arange(3).expand(collector.N, 3))
            else:
                league.assign(collector, make_net)                                          # resumed: :55-56

    def run_update(self):
        a, u = self.args, self.update_num
        if a.use_linear_lr_decay:                                                           # :98-99
            lr = linear_lr(u, self.num_updates, a.lr)
            for g in self.trainer.optimiser.param_groups:
                g["lr"] = lr
        if getattr(a, "teacher", None) is not None:       # kickstarting: this update's coefficient; once it is 0 nothing more is launched
            coef = teacher_coef_at(u, a)
            if coef > 0 and getattr(self.collector, "teacher", None) is None:
                raise ValueError("TrainArgs.teacher needs a collector built with RolloutCollector(teacher=train_loop.make_teacher(args, env))")
            self.trainer.cfg.teacher_coef = coef
            self.trainer.cfg.teacher_only = bool(coef > 0 and u < a.teacher_only_updates)
            if not coef > 0 and getattr(self.collector, "teacher", None) is not None:
                stop = getattr(self.collector, "stop_teacher", None)      # (frees the label tensor too)
                if stop is not None:
                    stop()
                else:
                    self.collector.teacher = None
        st = self.collector.gather_rollouts()                                               # :101-102
        league_totals, league_out = self._record_league(st), None
        losses = self.trainer.update(st)                                                    # :104
        self.collector.after_rollouts()
        self.entropy_coef = entropy_coef_at(u, a, self.entropy_coef)
        self.trainer.cfg.entropy_coef = self.entropy_coef
        w = reward_weight_at(u, a, self.reward_weight)
        if w != self.reward_weight:
            self.reward_weight = w
            self.env.set_reward_annealing_factor(w)                                             # rollout_manager.update_annealing_factor
        if self.league is not None:
            if u % a.add_policy_every == 0 and u > 0:                                       # :135-138
                self.league.add(self.policy)
            if league_totals is not None:     # the scoreboard as the draw below finds it: this rollout on record, this update's snapshot in
                lg = self.league
                league_out = {"serials": lg.serials(), "pairs": [float(lg.records[s][1]) if s in lg.records else 0.0 for s in lg.serials()],
                              "central_share": [float(x) for x in lg.central_share()],
                              "probabilities": [float(x) for x in lg.probabilities()], "totals": league_totals}
            if u % a.update_opponent_policies_every == 0:                                   # :140-141
                self.league.assign(self.collector, self.make_net)
        summary = None
        if self.evaluate is not None and u % a.eval_every == 0 and u > 0:                   # :143-151
            log, summary = self.evaluate(self.policy, u)
            self.eval_logs.append(log)
        self.update_num += 1
        if self.checkpoint_path and (not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0):
            self.save(self.checkpoint_path)                                                 # :155-156
        out = {"update": u, "losses": losses, "games_complete": st.games_complete, "entropy_coef": self.entropy_coef,
               "reward_weight": self.reward_weight, "policy_steps": self.steps_per_update * (u + 1),
               "hours": (time.time() - self.start_time) / 3600.0, "eval": summary}
        if getattr(st, "episode_stats", None) is not None:       # RolloutCollector(episode_stats=True): the games this rollout finished
            out["episodes"] = st.episode_stats
        if getattr(st, "records", None) is not None:             # RolloutCollector(record_games=k): the recorded games this rollout ended
            out["records"] = st.records
        if getattr(st, "start_pool", None) is not None:          # a start pool is installed: how this rollout's deals began
            sp = st.start_pool
            out["start_pool"] = {"pool": int(sp["pool"]), "fresh": int(sp["fresh"]), "per_entry": [int(x) for x in sp["per_entry"]]}
            if sp.get("outcomes") is not None:                   # ... and, with start_pool_outcomes, who won the games that began at each entry
                oc = sp["outcomes"]
                out["start_pool"]["outcomes"] = {"seen": int(oc["seen"]), "skipped": int(oc["skipped"]), "fresh": dict(oc["fresh"]),
                                                 "table": [[int(x) for x in row] for row in oc["table"]]}
        if league_out is not None:                               # RolloutCollector(league_stats=True): the scoreboard per snapshot
            out["league"] = league_out
        if getattr(self.trainer, "diagnostics", None) is not None:   # PPOConfig(diagnostics=True): what the clipped objective did in this update
            out["ppo"] = self.trainer.diagnostics
        if getattr(self.trainer, "teacher", None) is not None:       # PPOConfig(teacher_coef > 0): the update's imitation read-out
            out["teacher"] = self.trainer.teacher
        return out

    def _record_league(self, st):
        """The rollout's league table (RolloutCollector(league_stats=True)) goes on the league's record, summed over the ranks.  -> its
        totals row as a dict, or None: no table, no league, or opponents the league did not draw (the first rollout's random-initialised
        nets are no snapshots)."""
        table = getattr(st, "league_stats", None)
        if table is None or self.league is None or getattr(self.league, "in_play", None) is None:
            return None
        reduce = None
        if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            def reduce(dense):
                t = dense.to("cuda" if torch.distributed.get_backend() == "nccl" else "cpu")
                torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM)
                return t.cpu()
        self.league.record(table, reduce=reduce)
        return {k: int(v) for k, v in zip(spec.LEAGUE_STATS_TOTALS, torch.as_tensor(table)[-1].tolist())}

    def save(self, path):
        ck = {"central_policy": {k: v.detach().cpu() for k, v in self.policy.state_dict().items()},
              "earlier_policies": list(self.league.earlier) if self.league is not None else [],
              "eval_logs": self.eval_logs, "update_num": self.update_num, "args": copy.copy(self.args.__dict__),
              "entropy_coef": self.entropy_coef, "reward_weight": self.reward_weight}
        # (only where the scoreboard is in use: without it a checkpoint holds what it always held)
        if self.league is not None and (getattr(self.league, "records", None) or getattr(self.collector, "league_stats", False)):
            ck["league_serials"] = self.league.serials()
            ck["league_records"] = {int(s): [float(x) for x in r] for s, r in self.league.records.items()}
        torch.save(ck, path)

    def save_reference_tuple(self, path):
        """The reference's own checkpoint layout (robust_train.py:155-156): the 5-tuple (central state-dict, deque of
        earlier state-dicts, eval logs, update number, args).  State-dict keys are the reference's (CatanPolicy keeps its
        parameter names); the reference's entries without learnable state (the empty `dummy_param`s of its sub-modules, the
        value normaliser's constants) are added to the central state-dict AND to every league entry, so that the reference's
        strict `load_state_dict` accepts them (`policy.CatanPolicy.to_reference_state_dict`)."""
        import argparse
        from collections import deque
        complete = getattr(type(self.policy), "to_reference_state_dict", None) or (lambda d: {k: v.detach().cpu() for k, v in d.items()})
        sd = complete(self.policy.state_dict())
        earlier = deque((complete(e) for e in (self.league.earlier if self.league is not None else [])),
                        maxlen=(self.league.earlier.maxlen if self.league is not None else 500))
        torch.save((sd, earlier, self.eval_logs, self.update_num, argparse.Namespace(**self.args.__dict__)), path)

    def load_reference_tuple(self, path):
        """robust_train.py:55: accepts the reference's 5-tuple (or its 7-tuple variant with entropy coefficient and reward weight)."""
        ck = torch.load(path, map_location="cpu", weights_only=False)
        sd, earlier, self.eval_logs, self.update_num = ck[0], ck[1], ck[2], ck[3]
        own = self.policy.state_dict()
        self.policy.load_state_dict({k: v for k, v in sd.items() if k in own})
        if self.league is not None:
            self.league.earlier.clear()
            self.league.earlier.extend({k: v for k, v in e.items() if k in own} for e in earlier)
            self.league.assign(self.collector, self.make_net)
        if len(ck) >= 7:
            self.entropy_coef, self.reward_weight = ck[5], ck[6]
            self.trainer.cfg.entropy_coef = self.entropy_coef
            self.env.set_reward_annealing_factor(self.reward_weight)

    def load(self, path):
        ck = torch.load(path, map_location="cpu", weights_only=False)
        self.policy.load_state_dict(ck["central_policy"])
        if self.league is not None:
            self.league.earlier.clear(); self.league.earlier.extend(ck["earlier_policies"])
            if "league_serials" in ck and hasattr(self.league, "restore"):                  # (absent in older checkpoints: numbered afresh, no records)
                self.league.restore(ck["league_serials"], ck.get("league_records", {}))
            self.league.assign(self.collector, self.make_net)                               # :55-56
        self.eval_logs, self.update_num = ck["eval_logs"], ck["update_num"]
        self.entropy_coef, self.reward_weight = ck["entropy_coef"], ck["reward_weight"]
        self.trainer.cfg.entropy_coef = self.entropy_coef
        self.env.set_reward_annealing_factor(self.reward_weight)
