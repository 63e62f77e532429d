"""In-training evaluation protocol, batched (reference RL/ppo/evaluation_manager.py:12-84, RL/ppo/run_evaluation_protocol.py,
RL/ppo/vec_evaluation.py; draw cap of evaluation/evaluation_manager.py:119).

The reference plays `num_eval_episodes` games in 16 worker processes: policy 0 (the central policy) against three copies
of an opponent policy (a random-initialised net in the protocol), a fresh random seat order per game
(`random.shuffle(order)`; policy i plays seat order[i]), sampling actions (`deterministic=False`), and logs the fraction of
games policy 0 won, the mean game length, the mean number of policy-0 decisions and policy 0's mean victory points.
Here all episodes run at once on one batched env (no auto-reset; finished games idle), one batched forward per distinct
net per pass.  The deciding player is the env's (discarder > trade target > players_go, evaluation_manager.py:76-84)."""
import random as _py_random

import numpy as np
import torch

from . import acting, spec
from .forward_search import export_games

PLAYER_IDS = [2, 4, 3, 1]            # [Blue, Red, Orange, White] - the list the reference shuffles (evaluation_manager.py:27)


def sample_orders(n_games, rng=None):
    """-> int64 [n_games, 4]: order[g][i] = PlayerId played by policy i in game g (`random.shuffle(self.order)` per game)."""
    rng = rng or _py_random
    out = np.zeros((n_games, 4), dtype=np.int64)
    for g in range(n_games):
        o = list(PLAYER_IDS)
        rng.shuffle(o)
        out[g] = o
    return out


def _stats_of(res, rows, dev):
    """act_fn's return value -> (actions, extras): a tensor of actions, or a dict with "actions" and any of "entropy",
    "value", "logp" ([rows]) and "head_log" ([rows, 4]); missing statistics are zeros"""
    if torch.is_tensor(res):
        res = {"actions": res}
    z = torch.zeros(rows, dtype=torch.float32, device=dev)
    ex = {k: (torch.as_tensor(res[k], device=dev).float().reshape(rows) if k in res else z) for k in ("entropy", "value", "logp")}
    ex["head_log"] = torch.as_tensor(res["head_log"], device=dev).float().reshape(rows, 4) if "head_log" in res else torch.zeros((rows, 4), device=dev)
    return res["actions"], ex


@torch.no_grad()
def run_evaluation_episodes(env, nets, orders, max_steps=None, deterministic=False, generator=None, autocast_dtype=None,
                            act_fn=None, assignment=None, stats=False, detailed=False, searchers=None, record=None,
                            start_blobs=None, check_blobs=False):
    """env: freshly reset games, auto_reset off.  nets: the policies (entries may be the same object; equal objects share a
    forward); without `assignment` four of them, policy i = nets[i] in every game.  assignment int [n,4] (optional): game g's
    policy i is nets[assignment[g][i]] (the offline evaluator's opponents drawn per game).  orders int [n,4].  max_steps: the
    offline evaluator's draw cap (2 500; None = play to the end).
    act_fn(net, idx, f, lists, lens, masks) -> actions [len(idx),18], or a dict of "actions" and optionally "entropy", "value",
    "logp", "head_log" (see _stats_of): replaces net.act on the rows idx (test hook).
    -> dict of numpy arrays: winner (policy index, -1 = draw), victory_points (of policy 0), game_steps, policy_decisions.
    stats: also, over policy 0's decisions (evaluation/evaluation_manager.py:44-134), tallied on the device inside the loop:
    entropy (per game: mean of the decisions' entropies; NaN without decisions), value (mean value), action_types (int [n, 13]
    counts), type_log_probs (per game: the list of (action type, joint log-prob) tuples); detailed: also head_logs (per game:
    the log_specific_action_output tuples of all its decisions, reference_api.head_log_tuples).
    searchers {policy index: forward_search.ForwardSearch (n_roots >= n)}: that policy's decisions are searched
    (evaluation/evaluation_manager.py:83-96).  In every pass the running games it decides are collected on the device and decided
    by `searcher.act(env, games=idx, initial_settlement=flag, ...)`; `initial_settlement` is true when the deciding player has placed
    no initial settlement, or one settlement and one road (:85-88).  A searched decision of policy 0 counts as a decision and its
    action type is tallied; its entropy, log-prob and value are 0.0 (:94-96).  LSTM nets: the planner gets all four seats' states of
    its games and returns its own next state (:90-93,108); `searcher.zero_opponent_hidden_states` and `searcher.max_thinking_time`
    (attributes, optional) are passed on.
    record=k: games 0..k-1 are recorded from their reset (VecCatanEnv.enable_recording / arm_recording) and returned as "records", a list
    of record.GameRecord in game order (a game stopped by max_steps has no final blob); the env's recorder is switched off again.
    None: no such key.
    start_blobs [m, 736] (numpy, tensor or a start_pool.StartPool): game g starts from start_blobs[g % m] instead of its
    deal, by env.import_state - no kernel of its own, the env runs without auto-reset.  An imported blob brings its own draw counter:
    two runs on envs with the same seed and the same blobs see the same dice for as long as the same actions are played, which is what
    makes a comparison of two policies from common positions a PAIRED one.  A record (record=k) then starts from the imported position.
    None: nothing is imported.
    check_blobs: the start blobs go through the state check before they are imported (VecCatanEnv.import_state(check=True)): a ValueError
    names those that break a rule.  The default launches nothing new."""
    n, dev = env.n, env.device
    if start_blobs is not None:
        b = getattr(start_blobs, "blobs", start_blobs)
        b = (b.cpu() if torch.is_tensor(b) else torch.from_numpy(np.array(b, dtype=np.int32))).to(torch.int32).reshape(-1, spec.STATE_WORDS)
        if b.shape[0] < 1:
            raise ValueError("start_blobs: at least one position")
        picked = b[torch.arange(n) % b.shape[0]]
        if check_blobs:
            env.import_state(picked, check=True)
        else:
            env.import_state(picked)
    if record:
        env.enable_recording(list(range(int(record))))
        env.arm_recording()
    orders_t = torch.as_tensor(orders, device=dev).long()
    policy_of_pid = torch.empty((n, 4), dtype=torch.long, device=dev)
    policy_of_pid.scatter_(1, orders_t - 1, torch.arange(4, device=dev).expand(n, 4))
    if autocast_dtype is not None:        # weights in the autocast dtype: no per-call casts (policy.inference_copy)
        cache = {}
        nets = [cache.setdefault(id(n), n.inference_copy(autocast_dtype)) if (hasattr(n, "inference_copy") and getattr(n, "_inference_dtype", None) is None)
                else n for n in nets]
    distinct = []
    for net in nets:
        if not any(net is d for d in distinct):
            distinct.append(net)
    distinct_of = [[i for i, d in enumerate(distinct) if d is net][0] for net in nets]
    if assignment is None:
        assert len(nets) == 4
        assignment = np.broadcast_to(np.arange(4), (n, 4))
    assignment = np.asarray(assignment, dtype=np.int64)
    net_of = np.asarray(distinct_of, dtype=np.int64)[assignment]                 # [n, 4]: distinct net of game g's policy i
    net_of_policy = torch.as_tensor(net_of, device=dev)
    stats = stats or detailed
    stats_nets = set(int(k) for k in np.unique(net_of[:, 0])) if stats else set()  # the nets that play policy 0 somewhere
    if stats:
        ent_sum = torch.zeros(n, dtype=torch.float64, device=dev); val_sum = torch.zeros(n, dtype=torch.float64, device=dev)
        type_counts = torch.zeros((n, 13), dtype=torch.long, device=dev)
        trace_typ, trace_lp, trace_rec, trace_act = [], [], [], []
    ar = torch.arange(n, device=dev)
    steps = torch.zeros(n, dtype=torch.long, device=dev)
    decisions = torch.zeros(n, dtype=torch.long, device=dev)
    running = torch.ones(n, dtype=torch.bool, device=dev)
    draw = torch.zeros(n, dtype=torch.bool, device=dev)
    # LSTM policies: one (h, c) per seat, zero at the start of the game (evaluation_manager.py:20-26,50-59); a net without
    # an LSTM ignores its seats' entries.  The terminal mask stays 1: a finished evaluation game takes no further step.
    sizes = [int(net.lstm_size) for net in distinct if getattr(net, "include_lstm", False)]
    searchers = {int(k): v for k, v in (searchers or {}).items()}
    sizes += [int(sr.policy.lstm_size) for sr in searchers.values() if getattr(getattr(sr, "policy", None), "include_lstm", False)]
    hid = torch.zeros((2, n, 4, max(sizes)), dtype=torch.float32, device=dev) if sizes else None
    off_is, _ = spec.STATE_OFFSETS["init_settlements"]; off_ir, _ = spec.STATE_OFFSETS["init_roads"]
    while bool(running.any()):
        deciding = env.deciding_player().long()
        pol = policy_of_pid[ar, deciding - 1]
        f, lists, lens = env.get_obs()
        masks = env.get_action_masks()
        actions = torch.zeros((n, spec.ACTION_WORDS), dtype=torch.int64, device=dev)
        net_id = net_of_policy[ar, pol]
        if stats:
            ent_p = torch.zeros(n, device=dev); val_p = torch.zeros(n, device=dev); lp_p = torch.zeros(n, device=dev)
            rec_p = torch.zeros((n, 4), device=dev)
        searched = torch.zeros(n, dtype=torch.bool, device=dev)
        for p, sr in searchers.items():
            idx = (running & (pol == p)).nonzero(as_tuple=True)[0]
            if idx.numel() == 0:
                continue
            searched[idx] = True
            seat = deciding[idx] - 1
            blob = export_games(env, idx)        # (the whole 2 944-byte blob for two of its words per game: small beside a search)
            ar_i = torch.arange(idx.numel(), device=dev)
            n_set, n_road = blob[ar_i, off_is + seat], blob[ar_i, off_ir + seat]
            flag = (n_set == 0) | ((n_set == 1) & (n_road == 1))                      # evaluation_manager.py:85-88
            kw = {"games": idx, "initial_settlement": flag.cpu().numpy(), "deterministic": deterministic}
            if getattr(sr, "max_thinking_time", None) is not None:
                kw["max_thinking_time"] = sr.max_thinking_time
            rec = bool(getattr(getattr(sr, "policy", None), "include_lstm", False))
            if rec:
                L = int(sr.policy.lstm_size)
                zero = bool(getattr(sr, "zero_opponent_hidden_states", False))
                kw.update(hidden=hid[:, idx, :, :L].clone(), zero_opponent_hidden_states=zero)
                if zero:
                    # The reference planner writes the zeros into the dict it was handed (policy.py:81-86), and that dict is the
                    # manager's own current_hidden_states: the opponents' REAL states are wiped at every searched decision,
                    # single-proposal decisions included (the zeroing precedes the shortcut at policy.py:89).  The planner's own
                    # row is replaced by its next state below.
                    own = torch.zeros((idx.numel(), 4), dtype=torch.bool, device=dev)
                    own[ar_i, seat] = True
                    hid[:, idx] = hid[:, idx] * own[None, :, :, None]
            chosen, info = sr.act(env, **kw)
            actions[idx] = torch.as_tensor(chosen, device=dev).long()
            if rec:
                nh = info["next_hidden"].to(dev).float()                              # [2, r, L] (:108)
                hid[0, idx, seat, :L], hid[1, idx, seat, :L] = nh[0], nh[1]
        for k, net in enumerate(distinct):
            idx = ((net_id == k) & running & ~searched).nonzero(as_tuple=True)[0]
            if idx.numel() == 0:
                continue
            args = (f[idx], lists[idx], lens[idx].long(), masks[idx])
            want = k in stats_nets
            if act_fn is not None:
                actions[idx], ex = _stats_of(act_fn(net, idx, *args), idx.numel(), dev)
                if want:
                    ent_p[idx], val_p[idx], lp_p[idx], rec_p[idx] = ex["entropy"], ex["value"], ex["logp"], ex["head_log"]
                continue
            kw = {"deterministic": deterministic, "generator": generator}
            if getattr(net, "wants_games", False):       # a policy that reads the games themselves (scripted.ScriptedPolicy): row j is game idx[j];
                kw["games"] = idx                        # no entropy, no head log - as policy 0 its statistics are zeros, as a searched decision's
                want = False
            if want:
                kw.update(return_entropy=True, return_head_log=detailed)
            rec = getattr(net, "include_lstm", False)
            if rec:
                L, seat = int(net.lstm_size), deciding[idx] - 1
                kw.update(hidden=(hid[0, idx, seat, :L], hid[1, idx, seat, :L]), nonterminal=torch.ones(idx.numel(), device=dev))
            res = acting.act(net, args, autocast_dtype, **kw)
            actions[idx] = res[1]
            if rec:
                hid[0, idx, seat, :L], hid[1, idx, seat, :L] = res[3][0].float(), res[3][1].float()
            if want:
                j = 4 if rec else 3
                ent_p[idx], val_p[idx], lp_p[idx] = res[j].float(), res[0].float().reshape(-1), res[2].float().reshape(-1)
                if detailed:
                    rec_p[idx] = res[j + 1].float()
        if stats:                                        # policy 0's decisions of this pass, on the device
            p0 = running & (pol == 0)
            ent_sum += torch.where(p0, ent_p, torch.zeros_like(ent_p)).double()
            val_sum += torch.where(p0, val_p, torch.zeros_like(val_p)).double()
            type_counts.index_put_((ar, actions[:, 0].clamp(0, 12)), p0.long(), accumulate=True)
            trace_typ.append(torch.where(p0, actions[:, 0], torch.full_like(actions[:, 0], -1)).to(torch.int8))
            trace_lp.append(lp_p)
            if detailed:
                trace_rec.append(rec_p); trace_act.append(actions[:, :7].to(torch.int8))
        a_env = actions.to(torch.int32)
        a_env[:, 0] = torch.where(running, a_env[:, 0], torch.full_like(a_env[:, 0], -1))
        _, done = env.step(a_env)
        decisions += (running & (pol == 0)).long()
        steps += running.long()
        done = done.bool() & running
        if max_steps is not None:
            capped = running & ~done & (steps > max_steps)                    # `if total_game_steps > 2500: DRAW`
            draw |= capped
            done = done | capped
        running &= ~done
    blob = env.export_state()
    off_w, _ = spec.STATE_OFFSETS["winner"]; off_v, _ = spec.STATE_OFFSETS["curr_vps"]
    winner_pid = blob[:, off_w].long()
    winner = torch.where(draw, torch.full_like(winner_pid, -1), policy_of_pid[ar, (winner_pid - 1).clamp(min=0)])
    vps = blob[:, off_v:off_v + 4].long()[ar, orders_t[:, 0] - 1]             # env.curr_vps[self.order[0]]
    out = {"winner": winner.cpu().numpy(), "victory_points": vps.cpu().numpy(), "game_steps": steps.cpu().numpy(),
           "policy_decisions": decisions.cpu().numpy()}
    if stats:
        out.update(_stats_result(decisions, ent_sum, val_sum, type_counts, trace_typ, trace_lp, trace_rec, trace_act, detailed))
    if record:
        out["records"] = env.recordings(sealed_only=False)
        env.enable_recording([])
    return out


def _stats_result(decisions, ent_sum, val_sum, type_counts, trace_typ, trace_lp, trace_rec, trace_act, detailed):
    """the device tallies -> the per-game statistics (one copy to the host at the end)"""
    dec = decisions.double()
    with np.errstate(invalid="ignore", divide="ignore"):
        ent = (ent_sum / dec).cpu().numpy(); val = (val_sum / dec).cpu().numpy()
    typ = torch.stack(trace_typ, 1).cpu().numpy()                               # [n, passes], -1: not a policy-0 decision
    lp = torch.stack(trace_lp, 1).cpu().numpy()
    n = typ.shape[0]
    g, p = np.nonzero(typ >= 0)                                                 # row-major: per game in pass order
    bounds = np.searchsorted(g, np.arange(n + 1))
    t_all, l_all = typ[g, p].tolist(), lp[g, p]
    tuples = [[(t_all[i], l_all[i]) for i in range(bounds[k], bounds[k + 1])] for k in range(n)]
    out = {"entropy": ent, "value": val, "action_types": type_counts.cpu().numpy(), "type_log_probs": tuples}
    if detailed:
        from .reference_api import head_log_tuples_np
        rec = torch.stack(trace_rec, 1).cpu().numpy()[g, p]
        act = torch.stack(trace_act, 1).cpu().numpy()[g, p]
        out["head_logs"] = [[t for i in range(bounds[k], bounds[k + 1]) for t in head_log_tuples_np(rec[i], act[i])] for k in range(n)]
    return out


def _protocol_entry(res):
    return {"policy_win_frac": float(np.mean(res["winner"] == 0)), "avg_game_length": float(np.mean(res["game_steps"])),
            "avg_policy_decisions": float(np.mean(res["policy_decisions"])), "avg_victory_points": float(np.mean(res["victory_points"]))}


def _protocol_paragraph(name, num_eval_episodes, res, r):
    return ("{} games against {}. Policy won {}/{}. Avg. game length: {}. Avg num policy decisions: {}. "
            "Avg victory points for policy: {}. \n\n").format(num_eval_episodes, name, int(np.sum(res["winner"] == 0)), num_eval_episodes,
                                                             r["avg_game_length"], r["avg_policy_decisions"], r["avg_victory_points"])


def run_evaluation_protocol(make_env, central_policy, opponent_policy, num_eval_episodes, update_num=0, rng=None, baselines=None, **kw):
    """run_evaluation_protocol.py: the central policy against three copies of `opponent_policy` (the protocol's "random"
    opponent).  make_env(n) -> n freshly reset games without auto-reset.  -> (log dict, summary string).
    baselines {name: policy}: fixed opponents beside the protocol's (e.g. {"scripted": scripted.ScriptedPolicy} - the class or an
    instance); for each, the same number of episodes is played against three copies of it, on a fresh env it is bound to
    (`rebind`), after the protocol's own games; log[name] holds the four keys of log["random"], the summary one more paragraph.
    None: the reference's protocol and nothing else."""
    env = make_env(num_eval_episodes)
    res = run_evaluation_episodes(env, [central_policy, opponent_policy, opponent_policy, opponent_policy],
                                  sample_orders(num_eval_episodes, rng), **kw)
    log = {"update": update_num, "random": _protocol_entry(res)}
    if "records" in res:                  # run_evaluation_episodes(record=k): per opponent, under the opponent's name
        log["records"] = {"random": res["records"]}
    summary = ("\n\n---------------------- EVALUATION (after {} updates) ----------------------\n".format(update_num)
               + _protocol_paragraph("random", num_eval_episodes, res, log["random"]))
    for name, base in (baselines or {}).items():
        if name in log:
            raise ValueError(f"run_evaluation_protocol: the baseline name {name!r} is taken by the protocol's own log")
        env = make_env(num_eval_episodes)
        base = base() if isinstance(base, type) else base
        if hasattr(base, "rebind"):
            base.rebind(env)
        res = run_evaluation_episodes(env, [central_policy, base, base, base], sample_orders(num_eval_episodes, rng), **kw)
        log[name] = _protocol_entry(res)
        if "records" in res:
            log["records"][name] = res["records"]
        summary += _protocol_paragraph(name, num_eval_episodes, res, log[name])
    return log, summary


def run_forward_search_evaluation(planner, other_policies, num_games, make_env=None, make_sim_env=None, seed=10, deterministic=False,
                                  out_file="forward_policy_evaluation.pt", max_steps=2500, autocast_dtype=None, record=None):
    """evaluation/run_forward_search_evaluation.py: policy 0 is the planner (`reference_api.ForwardSearchPolicy`), the other
    three seats are the nets `other_policies`; all num_games games run at once.  make_env(n) -> n freshly reset games without
    auto-reset (default: VecCatanEnv on the planner's device).  Prints the fraction of games the planner won and saves the
    reference's tuple (winners, game steps, victory points, planner decisions, sorted action-type counts) to out_file
    (None: not saved).  record=k: the first k games are recorded (run_evaluation_episodes).  -> the dict of run_evaluation_episodes(stats=True)."""
    if make_env is None:
        from .env import VecCatanEnv
        make_env = lambda n: VecCatanEnv(n, seed=seed, auto_reset=False, device=planner._device)  # noqa: E731
    env = make_env(num_games)
    searcher = planner.make_searcher(num_games, make_sim_env)
    res = run_evaluation_episodes(env, [planner.base_policy] + list(other_policies), sample_orders(num_games, _py_random.Random(seed)),
                                  max_steps=max_steps, deterministic=deterministic, autocast_dtype=autocast_dtype, stats=True,
                                  searchers={0: searcher}, record=record)
    print("{} games finished. Fraction of games won by forward search: {}".format(num_games, float(np.mean(res["winner"] == 0))))
    if out_file is not None:
        counts = res["action_types"].sum(0)
        torch.save(([int(w) for w in res["winner"]], [int(x) for x in res["game_steps"]], [int(x) for x in res["victory_points"]],
                    [int(x) for x in res["policy_decisions"]], sorted((int(t), int(c)) for t, c in enumerate(counts) if c)), out_file)
    return res
