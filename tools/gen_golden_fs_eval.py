"""Generates tests/golden/fs_eval_small.npz and tests/golden/forward_search_flags.npz from the imported upstream reference
(development container only; data in, data out - no reference source is stored).

  fs_eval_small.npz         the reference's `evaluation/evaluation_manager.py::EvaluationManager.run_evaluation_game` on N_GAMES full
                            games with patched Philox streams and scripted decisions (ref_harness, as gen_golden.gen_eval_small).
                            policies[0] is a scripted stand-in with policy_type "forward_search": its `act` plays the scripted
                            action and records what the manager handed it (`initial_settlement`, `decision_no`).  Per game g:
                              g{g}_order            PlayerId of policy i (the shuffled order)
                              g{g}_result           winner, victory points, game steps, planner decisions
                              g{g}_entropy / _value the means the manager returns (the planner's decisions enter as 0.0)
                              g{g}_action_types     int [13] counts of the planner's action types
                              g{g}_type_log_probs   float64 [decisions, 2]: the (type, log-prob) tuples
                              g{g}_flags            int [planner calls, 3]: index of the call in the all-seat trace, initial_settlement, decision_no
                              g{g}_trace            every decision of every seat;  g{g}_final_blob  the final state
                            The random.seed of every game is chosen so that the planner plays a different PlayerId (and sits in a
                            different seat of the turn order) in each game.
  forward_search_flags.npz  `default_sample_actions` on the proposal inputs of forward_search.npz (regenerated the same way and
                            checked equal to the stored ones) with dont_propose_devcards, dont_propose_trades and both:
                            dev_* / trade_* / both_* = count per input and the concatenated proposal lists; count -1 = the reference
                            raises there (UnboundLocalError at sample_actions_fn.py:154: no earlier proposal to repeat).
                            x_*: three fresh inputs generated the same way (PlayDevelopmentCard legal next to a building proposal,
                            BuyDevelopmentCard legal), with their inputs and the lists of the plain call (x_none_*) and of the three.

usage: python tools/gen_golden_fs_eval.py"""
import copy
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402  (puts the reference on sys.path)

OUT = os.path.join(ROOT, "tests", "golden")
N_GAMES = 3


class _Seat(object):
    """one entry of the manager's `policies`: the real net's converters, a scripted `act`"""

    def __init__(self, ctx, real, policy_type, flags):
        self.ctx, self.real, self.policy_type, self.flags = ctx, real, policy_type, flags
        self.lstm_size = real.lstm_size
        self.player_id = None

    def eval(self):
        return self

    def __getattr__(self, name):
        if name == "initialise_policy":
            raise AttributeError(name)
        return getattr(self.real, name)

    def _scripted(self):
        import torch
        c = self.ctx
        env = c.envs[c.cur]
        a = rh.weighted_legal_action(env.get_action_masks(), env, c.rngs[c.cur])
        c.trace[c.cur].append(np.array(a, dtype=np.int8))
        heads = rh.action_to_heads(a)
        return a, [[torch.tensor([[int(v)]]) for v in h] if isinstance(h, (list, np.ndarray)) else torch.tensor([[int(h)]]) for h in heads]

    def act(self, obs, hidden_states, third, action_masks, deterministic=False, return_entropy=False, decision_no=None, initial_settlement=None):
        import torch
        if self.policy_type == "forward_search":                     # (obs, all seats' states, saved env state, masks, decision_no=, initial_settlement=)
            assert isinstance(hidden_states, dict) and decision_no is not None
            self.flags.append((len(self.ctx.trace[self.ctx.cur]), int(bool(initial_settlement)), int(decision_no)))
            a, heads = self._scripted()
            return self.real.torch_act_to_np(heads), hidden_states[self.player_id]
        a, heads = self._scripted()
        assert return_entropy
        return torch.tensor([[1.5]]), heads, torch.tensor([[rh.scripted_log_prob(a)]], dtype=torch.float32), hidden_states, torch.tensor(0.75)


def _order_for(seed):
    from game.enums import PlayerId
    random.seed(seed)
    o = [PlayerId.Blue, PlayerId.Red, PlayerId.Orange, PlayerId.White]
    random.shuffle(o)
    return o


def gen_fs_eval_small(n_games=N_GAMES, seed=43):
    from evaluation.evaluation_manager import EvaluationManager
    out = {"seed": seed, "n_games": n_games}
    used_pid, used_seat, summary = set(), set(), []
    for g in range(n_games):
        # a random.seed under which the planner gets a PlayerId and a seat of the turn order that no earlier game gave it
        pyseed = 600 + 97 * g
        while True:
            with rh.patched_rng(rh.PhiloxStream(seed ^ 0xABC, g)):
                mgr = EvaluationManager()
            stream = rh.PhiloxStream(seed, g)
            ctx = rh.ScriptedContext([mgr.env], [stream], [7100 + g])
            ctx.hook_manager(mgr)
            real = mgr.policies[0]
            flags = []
            mgr.policies = [_Seat(ctx, real, "forward_search" if i == 0 else "neural_network", flags) for i in range(4)]
            random.seed(pyseed)
            res = mgr.run_evaluation_game()
            seat = [int(p) for p in mgr.env.game.player_order].index(int(mgr.order[0]))
            if int(mgr.order[0]) not in used_pid and seat not in used_seat:
                break
            pyseed += 1
        used_pid.add(int(mgr.order[0])); used_seat.add(seat)
        winner, vps, steps, decisions, entropy, action_types, type_lp, value = res
        out[f"g{g}_order"] = np.array([int(p) for p in mgr.order], dtype=np.int8)
        out[f"g{g}_result"] = np.array([winner, vps, steps, decisions], dtype=np.int32)
        out[f"g{g}_entropy"] = np.float64(entropy); out[f"g{g}_value"] = np.float64(value)
        cnt = np.zeros(13, dtype=np.int32)
        for t, c in action_types.items():
            cnt[int(t)] = c
        out[f"g{g}_action_types"] = cnt
        out[f"g{g}_type_log_probs"] = np.array([(float(t), float(lp)) for t, lp in type_lp], dtype=np.float64).reshape(-1, 2)
        out[f"g{g}_flags"] = np.array(flags, dtype=np.int32).reshape(-1, 3)
        out[f"g{g}_trace"] = np.array(ctx.trace[0], dtype=np.int8)
        out[f"g{g}_final_blob"] = rh.state_blob(mgr.env, stream.draws)
        out[f"g{g}_planner_seat"] = np.int32(seat)
        assert len(flags) == decisions and [f[2] for f in flags] == list(range(decisions)) and entropy == 0.0 and value == 0.0
        summary.append((int(mgr.order[0]), seat, int(winner), int(steps), int(decisions), int(sum(f[1] for f in flags))))
    path = os.path.join(OUT, "fs_eval_small.npz")
    np.savez_compressed(path, **out)
    return {"games (planner pid, seat, winner, steps, decisions, initial flags)": summary, "bytes": os.path.getsize(path)}


def gen_forward_search_flags():
    import torch
    import policy_fixture as pf
    import RL.models.build_agent_model as bam
    from RL.forward_search_policy.sample_actions_fn import default_sample_actions
    g = np.load(os.path.join(OUT, "forward_search.npz"))
    torch.manual_seed(0)
    ref_net = bam.build_agent_model(device="cpu")
    sd = ref_net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if v.numel() > 0 and not k.startswith("value_normaliser.")}
    full = dict(sd); full.update(pf.fixture_state_dict(shapes, "ff:"))
    ref_net.load_state_dict(full, strict=True)
    ref_net.eval()
    orig = ref_net.act
    ref_net.act = lambda *a, **kw: orig(*a, **{**kw, "deterministic": True})
    combos = {"dev": dict(dont_propose_devcards=True), "trade": dict(dont_propose_trades=True),
              "both": dict(dont_propose_devcards=True, dont_propose_trades=True)}
    wants = {k: [] for k in combos}
    changed_extra = {"dev": 0}
    dup_dev = {k: 0 for k in combos}      # inputs where the switch meets a legal PlayDevelopmentCard and the reference returns a list
    legal_dev = legal_trade = 0
    states = [(3, 0), (3, 5), (3, 60), (3, 300), (6, 700), (6, 1100), (9, 1500), (9, 2100), (12, 2500), (12, 40)]     # gen_golden.gen_forward_search
    for i, (seed, warm) in enumerate(states):
        rng = np.random.default_rng(seed + warm)
        ref = rh.RefEnv(seed, 0)
        obs = ref.reset()
        for _ in range(warm):
            obs, _, done = ref.step(rh.random_legal_action(ref.masks(), ref.env, rng))
            if done:
                obs = ref.reset()
        f, lists, lens, _ = rh.obs_flat(obs)
        m = rh.masks_flat(ref.masks())
        assert np.array_equal(g["prop_obs_f"][i].astype(np.float32), f) and np.array_equal(g["prop_lists"][i], lists.astype(np.int8))
        assert np.array_equal(np.unpackbits(g["prop_masks"][i], bitorder="little")[:325], m.astype(np.uint8))
        legal_dev += int(m[4] > 0); legal_trade += int(m[6] > 0)
        initial = bool(ref.env.game.initial_placement_phase)
        assert initial == bool(g["prop_initial"][i])
        for name, kw in combos.items():
            random.seed(1234 + warm)
            masks_t = ref_net.act_masks_to_torch(ref.env.get_action_masks())
            try:
                want, _ = default_sample_actions(ref_net.obs_to_torch(copy.deepcopy(obs)), None, masks_t, ref_net, 10, initial_settlement_phase=initial, **kw)
            except UnboundLocalError:
                # sample_actions_fn.py:154 appends the PREVIOUS proposal when the dev-card switch is on; with PlayDevelopmentCard legal and
                # no settlement / road / city proposal before it there is none.  Recorded as count -1.
                assert kw.get("dont_propose_devcards") and m[4] > 0 and not (m[0] > 0 or m[1] > 0 or m[2] > 0)
                wants[name].append(None)
                continue
            dup_dev[name] += int(bool(kw.get("dont_propose_devcards")) and m[4] > 0)
            wants[name].append(np.array([np.concatenate([np.asarray(h).reshape(-1) for h in a]) for a in want], dtype=np.int8).reshape(-1, 18))
    # fresh inputs, generated the same way: states where the dev-card switch meets a legal PlayDevelopmentCard next to a building
    # proposal (the repeated entry) and where BuyDevelopmentCard is legal; stored with the list of the plain call ("none")
    def lists_of(ref, obs, initial, pyseed, kw):
        random.seed(pyseed)
        masks_t = ref_net.act_masks_to_torch(ref.env.get_action_masks())
        want, _ = default_sample_actions(ref_net.obs_to_torch(copy.deepcopy(obs)), None, masks_t, ref_net, 10, initial_settlement_phase=initial, **kw)
        return np.array([np.concatenate([np.asarray(h).reshape(-1) for h in a]) for a in want], dtype=np.int8).reshape(-1, 18)
    extra = {k: [] for k in ("f", "lists", "lens", "masks", "initial", "seed", "none", "dev", "trade", "both")}
    need = {"play_next_to_build": 2, "buy": 1}
    for seed in range(21, 40):
        if not any(need.values()):
            break
        rng = np.random.default_rng(seed)
        ref = rh.RefEnv(seed, 0)
        obs = ref.reset()
        for step in range(2500):
            m = rh.masks_flat(ref.masks())
            kind = "play_next_to_build" if (m[4] > 0 and (m[0] > 0 or m[1] > 0 or m[2] > 0)) else ("buy" if m[3] > 0 else None)
            if kind is not None and need[kind] > 0 and step % 7 == 0:
                need[kind] -= 1
                f, lists, lens, _ = rh.obs_flat(obs)
                initial = bool(ref.env.game.initial_placement_phase)
                extra["f"].append(f); extra["lists"].append(lists); extra["lens"].append(lens); extra["masks"].append(m)
                extra["initial"].append(initial); extra["seed"].append(5000 + step)
                extra["none"].append(lists_of(ref, obs, initial, 5000 + step, {}))
                for name, kw in combos.items():
                    extra[name].append(lists_of(ref, obs, initial, 5000 + step, kw))
                dup_dev["dev"] += int(kind == "play_next_to_build"); dup_dev["both"] += int(kind == "play_next_to_build")
                assert not np.array_equal(extra["dev"][-1], extra["none"][-1]) or extra["dev"][-1].shape != extra["none"][-1].shape
                changed_extra["dev"] += 1
                legal_dev += int(m[4] > 0)
            obs, _, done = ref.step(rh.random_legal_action(ref.masks(), ref.env, rng))
            if done:
                obs = ref.reset()
    assert not any(need.values()), need
    assert legal_dev >= 1 and legal_trade >= 1, (legal_dev, legal_trade)
    out = {}
    out["x_obs_f"] = np.stack(extra["f"]).astype(np.float16); assert np.array_equal(out["x_obs_f"].astype(np.float32), np.stack(extra["f"]))
    out["x_lists"] = np.stack(extra["lists"]).astype(np.int8); out["x_lens"] = np.stack(extra["lens"]).astype(np.int8)
    out["x_masks"] = np.packbits(np.stack(extra["masks"]).astype(np.uint8), axis=1, bitorder="little")
    out["x_initial"] = np.array(extra["initial"], dtype=np.uint8); out["x_seed"] = np.array(extra["seed"], dtype=np.int64)
    for k in ("none", "dev", "trade", "both"):
        out["x_" + k + "_count"] = np.array([len(w) for w in extra[k]], dtype=np.int32)
        out["x_" + k + "_actions"] = np.concatenate(extra[k]).astype(np.int8)
    off = 0
    changed = {k: 0 for k in combos}
    for i, c in enumerate(g["prop_count"]):
        base = g["prop_actions"][off:off + c]; off += c
        for k in combos:
            changed[k] += int(wants[k][i] is not None and (wants[k][i].shape != base.shape or not np.array_equal(wants[k][i], base)))
    assert all(v + changed_extra.get(k, 0) >= 1 for k, v in changed.items()), changed
    assert dup_dev["dev"] >= 1 and dup_dev["both"] >= 1, dup_dev
    for k in combos:
        out[k + "_count"] = np.array([-1 if w is None else len(w) for w in wants[k]], dtype=np.int32)
        out[k + "_actions"] = np.concatenate([w for w in wants[k] if w is not None]).astype(np.int8)
    path = os.path.join(OUT, "forward_search_flags.npz")
    np.savez_compressed(path, **out)
    return {"legal play_dev": legal_dev, "legal prop_trade": legal_trade, "lists changed": changed, "counts": {k: out[k + "_count"].tolist() for k in combos},
            "bytes": os.path.getsize(path)}


if __name__ == "__main__":
    print("forward_search_flags", gen_forward_search_flags())
    print("fs_eval_small", gen_fs_eval_small())
