"""Generates the golden fixtures under tests/golden/ by driving the imported upstream reference
(development container only).  The fixtures are DATA (inputs + expected outputs); no reference source is stored.

  topology.npz        static board tables read from the reference Board
  reset_states.npz    post-reset state blobs for (seed, env_id) pairs under the philox contract (exercises the
                      6/8 rejection loop of board.py:79-81)
  traj_s{S}_e{E}.npz  random-policy trajectories: actions, rewards, dones, deciding player, packed masks and a crc32 of
                      the full state blob at EVERY step, full blobs + observations at sampled steps
  traj_rule_<case>.npz  rule-case trajectories (gen_rule_trajs): action lists scouted in the CPU oracle so that they reach a rule
                      branch the random trajectories never take, replayed and recorded by the reference (+ `event`, `event_step`)
  mt_kat.npz          the UNPATCHED reference under np.random.seed(s); random.seed(s) (global Mersenne Twisters):
                      actions + crc32 of the state at every step (config 1 known-answer test for the oracle MT mode)
  longest_road.npz    (edge_owner, corner_owner, player) -> Game.get_longest_path, harvested from play + adversarial
  gae_ppo.npz         BatchProcessor GAE / PPO loss values computed with the reference's torch code
  ppo_update.npz      two whole PPO.update calls of the reference (fp32 and fp64) on the fixture net: per optimiser step the
                      losses, the pre-clip norm, every parameter's gradient and theta_k - theta_0 (norms, hashed projections)
  ref_checks.npz      the reference's side of several parity checks (gen_ref_checks)
  validate_cases.npz  validate mode (Game.validate_action): states x probe actions -> the reference's accept / reject and,
                      for accepted ones, its state crc / masks / rewards / done afterwards (incl. actions outside the masks)
"""
import os
import sys
import zlib
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
from settlers_of_catan_rl_amd import spec  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def pack_masks(m):
    return np.packbits(m.astype(np.uint8), bitorder="little")


def gen_topology():
    env = rh.RefEnv(0, 0).env
    b = env.game.board
    K = ["T", "TL", "BL", "B", "BR", "TR"]
    EK = ["BL", "BR", "L", "R", "TL", "TR"]
    from game.enums import HARBOUR_CORNER_AND_EDGES, TILE_NEIGHBOURS
    np.savez_compressed(
        os.path.join(OUT, "topology.npz"),
        tile_corner=np.array([[b.tiles[t].corners[k].id for k in K] for t in range(19)], dtype=np.int32),
        tile_edge=np.array([[b.tiles[t].edges[k].id for k in EK] for t in range(19)], dtype=np.int32),
        edge_corner=np.array([(e.corner_1.id, e.corner_2.id) for e in b.edges], dtype=np.int32),
        corner_nbr_corner=np.array([[(n[0].id if n[0] is not None else -1) for n in c.corner_neighbours] for c in b.corners], dtype=np.int32),
        corner_nbr_edge=np.array([[(n[1].id if n[1] is not None else -1) for n in c.corner_neighbours] for c in b.corners], dtype=np.int32),
        corner_tile=np.array([[t.id if t is not None else -1 for t in c.adjacent_tiles] for c in b.corners], dtype=np.int32),
        harbour_slot_corner=np.array([[b.tiles[h[0]].corners[h[1]].id, b.tiles[h[0]].corners[h[2]].id]
                                      for h in [HARBOUR_CORNER_AND_EDGES[i] for i in range(9)]], dtype=np.int32),
        harbour_slot_edge=np.array([b.tiles[h[0]].edges[h[3]].id for h in [HARBOUR_CORNER_AND_EDGES[i] for i in range(9)]], dtype=np.int32),
        tile_nbr_mask=np.array([sum(1 << v for v in TILE_NEIGHBOURS[t].values()) for t in range(19)], dtype=np.int64),
        number_placement=np.array(b.NUMBER_PLACEMENT_INDS, dtype=np.int32),
    )


def gen_resets(n=192, seed=11):
    blobs = []
    for env_id in range(n):
        e = rh.RefEnv(seed, env_id)
        e.reset()
        blobs.append(e.state_blob())
    np.savez_compressed(os.path.join(OUT, "reset_states.npz"), seed=seed, blobs=np.array(blobs, dtype=np.int32))


def gen_traj(seed, env_id, steps, sample_every=97, name=None, dense=False, anneal=1.0, trades=4, max_actions=None,
             actions=None, also_sample=(), extra=None):
    """name/dense/anneal/trades/max_actions: EnvWrapper's non-default keyword arguments (env/wrapper.py:12-13: dense shaping
    :95-106 x env.reward_annealing_factor, trade limit :284-289, max_actions_per_turn :14-17,233-234); `rewards64` holds the
    reference's Python-float rewards.  The action source: the uniform-random legal policy (`actions` None), or a fixed list
    `actions` that is replayed (steps = its length; an action the reference's validate_action rejects raises).  `also_sample`:
    steps whose blob and observation are stored besides every sample_every-th; `extra`: further fields of the file."""
    rng = np.random.default_rng(seed * 7919 + env_id)
    replay = actions
    if replay is not None:
        steps = len(replay)
    source = (lambda t, e: rh.random_legal_action(e.masks(), e.env, rng)) if replay is None else (lambda t, e: np.asarray(replay[t], dtype=np.int32))
    also_sample = set(int(x) for x in also_sample)
    e = rh.RefEnv(seed, env_id, dense_reward=dense, max_proposed_trades_per_turn=trades, max_actions_per_turn=max_actions)
    e.env.reward_annealing_factor = anneal
    obs = e.reset()
    actions, rewards, dones, deciding, masks, crcs, rewards64 = [], [], [], [], [], [], []
    s_idx, s_blob, s_obs, s_lists, s_lens, s_pid = [], [], [], [], [], []
    for t in range(steps):
        blob = e.state_blob()
        m = rh.masks_flat(e.masks())
        crcs.append(crc(blob)); masks.append(pack_masks(m)); deciding.append(e.deciding_player())
        if t % sample_every == 0 or t in also_sample:
            f, lists, lens, pid = rh.obs_flat(obs)
            s_idx.append(t); s_blob.append(blob); s_obs.append(f); s_lists.append(lists); s_lens.append(lens); s_pid.append(pid)
        a = source(t, e)
        obs, rew, done = e.step(a)
        actions.append(a); rewards.append(rew); dones.append(done); rewards64.append(e.last_reward64)
        if done:
            obs = e.reset()
    np.savez_compressed(
        os.path.join(OUT, name or f"traj_s{seed}_e{env_id}.npz"), seed=seed, env_id=env_id,
        dense=int(dense), anneal=float(anneal), trades=-1 if trades is None else int(trades),
        max_actions=-1 if max_actions is None else int(max_actions), rewards64=np.array(rewards64, dtype=np.float64),
        actions=np.array(actions, dtype=np.int8), rewards=np.array(rewards, dtype=np.float32), dones=np.array(dones, dtype=np.uint8),
        deciding=np.array(deciding, dtype=np.int8), masks=np.array(masks, dtype=np.uint8), state_crc=np.array(crcs, dtype=np.uint32),
        sample_idx=np.array(s_idx, dtype=np.int32), sample_blob=np.array(s_blob, dtype=np.int16),
        sample_obs=np.packbits(np.array(s_obs) != 0, axis=1),        # observation: zero/non-zero pattern ...
        sample_obs_nz=np.concatenate([x[x != 0] for x in s_obs]).astype(np.float32),        # ... and the non-zero values
        sample_lists=np.array(s_lists, dtype=np.int8), sample_lens=np.array(s_lens, dtype=np.int8), sample_pid=np.array(s_pid, dtype=np.int8),
        final_blob=e.state_blob(), **(extra or {}))
    return int(np.sum(dones))


def gen_mt_kat(seeds=(0, 5), steps=1500):
    out = {}
    for s in seeds:
        np.random.seed(s); random.seed(s)
        env = rh.EnvWrapper()
        env.reset()
        arng = np.random.default_rng(1000 + s)
        acts, crcs = [], []
        for t in range(steps):
            crcs.append(crc(rh.state_blob(env, 0)))
            a = rh.random_legal_action(env.get_action_masks(), env, arng)
            _, _, done, _ = env.step(rh.action_to_heads(a))
            acts.append(a)
            if done:
                env.reset()
        out[f"actions_{s}"] = np.array(acts, dtype=np.int8)
        out[f"crc_{s}"] = np.array(crcs, dtype=np.uint32)
        out[f"final_{s}"] = rh.state_blob(env, 0)
    np.savez_compressed(os.path.join(OUT, "mt_kat.npz"), seeds=np.array(seeds), **out)


def gen_longest_road(n_play=400):
    """cases harvested from random play (states where roads exist) + adversarial synthetic networks, all evaluated by
    the reference Game.get_longest_path."""
    from game.enums import PlayerId
    from game.components.buildings import Building
    from game.enums import BuildingType
    cases_e, cases_c, cases_p, cases_len = [], [], [], []
    rng = np.random.default_rng(5)
    e = rh.RefEnv(21, 0)
    e.reset()
    g = e.env.game

    def record(pid):
        eo = [0 if ed.road is None else int(ed.road) for ed in g.board.edges]
        co = [0 if c.building is None else int(c.building.owner) for c in g.board.corners]
        if pid not in eo:
            return
        cases_e.append(eo); cases_c.append(co); cases_p.append(pid); cases_len.append(int(g.get_longest_path(PlayerId(pid))))

    t = 0
    while len(cases_len) < n_play:
        a = rh.random_legal_action(e.masks(), e.env, rng)
        _, _, done = e.step(a)
        t += 1
        if a[0] in (0, 1) and t % 3 == 0:
            for pid in (1, 2, 3, 4):
                record(pid)
        if done:
            e.reset(); g = e.env.game
    # adversarial: random dense networks with random opponent buildings (not reachable states, pure graph cases)
    for k in range(200):
        for ed in g.board.edges:
            ed.road = None
        for c in g.board.corners:
            c.building = None
        dens = rng.uniform(0.15, 0.6)
        for ed in g.board.edges:
            u = rng.random()
            if u < dens:
                ed.road = PlayerId(1)
            elif u < dens + 0.1:
                ed.road = PlayerId(2)
        for c in g.board.corners:
            if rng.random() < 0.12:
                c.building = Building(BuildingType.Settlement, PlayerId(int(rng.integers(1, 3))), c)
        eo = [0 if ed.road is None else int(ed.road) for ed in g.board.edges]
        if eo.count(1) > 26:        # keep the reference's exponential DFS tractable
            continue
        record(1)
    np.savez_compressed(os.path.join(OUT, "longest_road.npz"), edge_owner=np.array(cases_e, dtype=np.int8),
                        corner_owner=np.array(cases_c, dtype=np.int8), player=np.array(cases_p, dtype=np.int8),
                        length=np.array(cases_len, dtype=np.int8))


def gen_gae_ppo():
    """BatchProcessor.compute_advantages_alt lines 134-142 and PPO.update lines 54-66, run with the reference's own
    torch expressions on random tensors (fp32)."""
    import torch
    import types
    from RL.ppo.process_batch import BatchProcessor
    torch.manual_seed(0)
    out = {}
    for ci, (T, N) in enumerate([(7, 5), (50, 33), (200, 16)]):
        args = types.SimpleNamespace(num_steps=T, num_processes=N, num_envs_per_process=1, gamma=0.999, gae_lambda=0.95)
        bp = BatchProcessor(args, lstm_dim=4, device="cpu")
        bp.rewards = torch.where(torch.rand(T, N, 1) < 0.05, torch.full((T, N, 1), 500.0), torch.zeros(T, N, 1))
        bp.masks = (torch.rand(T + 1, N, 1) > 0.04).float()
        values = 150 + 150 * torch.randn(T + 1, N, 1) * 0.3

        class AC:   # feeds precomputed (normalised) values through the reference's own code path
            include_lstm = False
            use_value_normalisation = False

            def get_value(self, obs, h, m):
                return values[:, :obs["x"].shape[0] // (T + 1)] if False else None
        # run the exact reference lines 134-142 by calling the method with a stub that returns `values`
        bp.obs_keys = []
        bp.hidden_states = None
        ac = types.SimpleNamespace(include_lstm=False, use_value_normalisation=False)
        starts = {"i": 0}

        def get_value(obs_dict_in, rec, masks_in, _v=values):
            n_rows = masks_in.shape[0] // (T + 1)
            j = starts["i"]; starts["i"] += n_rows
            return _v[:, j:j + n_rows].reshape(-1, 1)
        ac.get_value = get_value
        bp.compute_advantages_alt(ac, 10)
        out[f"gae{ci}_rewards"] = bp.rewards[..., 0].numpy(); out[f"gae{ci}_values"] = values[..., 0].numpy()
        out[f"gae{ci}_masks"] = bp.masks[..., 0].numpy(); out[f"gae{ci}_returns"] = bp.returns[..., 0].numpy()
        out[f"gae{ci}_adv"] = bp.advantages[..., 0].numpy()
    # PPO loss, reference RL/ppo/ppo.py:54-63 verbatim semantics via torch autograd
    for ci, B in enumerate([64, 2000]):
        logp = (torch.randn(B, 1) * 0.5 - 3).requires_grad_(True)
        old = logp.detach() + torch.randn(B, 1) * 0.3
        adv = torch.randn(B, 1)
        v = torch.randn(B, 1).requires_grad_(True)
        v_old = v.detach() + torch.randn(B, 1) * 0.3
        ret = torch.randn(B, 1)
        clip = 0.2
        ratio = torch.exp(logp - old)
        surr1 = ratio * adv
        surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
        action_loss = -torch.min(surr1, surr2).mean()
        vpc = v_old + (v - v_old).clamp(-clip, clip)
        value_loss = 0.5 * torch.max((v - ret).pow(2), (vpc - ret).pow(2)).mean()
        (value_loss * 1.0 + action_loss).backward()
        for k, t in dict(logp=logp, old=old, adv=adv, v=v, v_old=v_old, ret=ret).items():
            out[f"ppo{ci}_{k}"] = t.detach().numpy()[:, 0]
        out[f"ppo{ci}_action_loss"] = action_loss.item(); out[f"ppo{ci}_value_loss"] = value_loss.item()
        out[f"ppo{ci}_dlogp"] = logp.grad.numpy()[:, 0]; out[f"ppo{ci}_dv"] = v.grad.numpy()[:, 0]
    # the reference's OWN PPO.update (RL/ppo/ppo.py:26-79) on one minibatch: stub storage + stub actor-critic whose values /
    # log-probs are parameters, so the hooks see d(loss)/d(values), d(loss)/d(log-probs) of lines 46-66 incl. the value
    # normaliser lines 46-48 (the reference's ValueFunctionNormaliser) and the returned (value, action, entropy) losses
    from RL.ppo.ppo import PPO
    from RL.models.utils import ValueFunctionNormaliser
    for ci, (B, use_norm) in enumerate([(96, True), (3000, True), (500, False)]):
        g = torch.Generator().manual_seed(100 + ci)
        lp0 = torch.randn(B, 1, generator=g) * 0.5 - 3
        v0 = torch.randn(B, 1, generator=g)
        old = lp0 + torch.randn(B, 1, generator=g) * 0.3
        adv = torch.randn(B, 1, generator=g)
        scale = (lambda x: 150 + 150 * x) if use_norm else (lambda x: x)
        v_old = scale(v0 + torch.randn(B, 1, generator=g) * 0.3)
        ret = scale(torch.randn(B, 1, generator=g))
        grads = {}

        class AC(torch.nn.Module):
            include_lstm = False

            def __init__(self):
                super().__init__()
                self.use_value_normalisation = use_norm
                self.value_normaliser = ValueFunctionNormaliser(mean=150.0, std=150.0)
                self.v = torch.nn.Parameter(v0.clone()); self.lp = torch.nn.Parameter(lp0.clone())
                self.ent = torch.nn.Parameter(torch.tensor(0.7))
                self.v.register_hook(lambda gr: grads.__setitem__("dv", gr.clone()))
                self.lp.register_hook(lambda gr: grads.__setitem__("dlogp", gr.clone()))

            def evaluate_actions(self, obs, rec, masks, actions, action_masks):
                return self.v * 1.0, self.lp * 1.0, self.ent * 1.0, None

        class Storage:
            num_parallel = 1; num_steps = B

            def compute_advantages_alt(self, ac, n):
                pass

            def generator_standard(self, num_mini_batch):
                yield ({}, None, None, None, v_old, ret, None, old, adv)

        a = types.SimpleNamespace(clip_param=0.2, ppo_epoch=1, num_mini_batch=1, value_loss_coef=0.5, entropy_coef_start=0.01,
                                  max_grad_norm=0.5, recompute_returns=True, gamma=0.999, gae_lambda=0.95, lr=1e-4, eps=1e-5, truncated_seq_len=10)
        agent = PPO(AC(), a)
        vl, al, el = agent.update(Storage())
        for k, t in dict(logp=lp0, old=old, adv=adv, v=v0, v_old=v_old, ret=ret).items():
            out[f"ppoU{ci}_{k}"] = t.numpy()[:, 0]
        out[f"ppoU{ci}_value_loss_x_coef"] = vl; out[f"ppoU{ci}_action_loss"] = al; out[f"ppoU{ci}_entropy_x_coef"] = el
        out[f"ppoU{ci}_dlogp"] = grads["dlogp"].numpy()[:, 0]; out[f"ppoU{ci}_dv"] = grads["dv"].numpy()[:, 0]
        out[f"ppoU{ci}_use_norm"] = np.int32(use_norm)
    out["ppoU_value_loss_coef"] = 0.5; out["ppoU_clip"] = 0.2
    np.savez_compressed(os.path.join(OUT, "gae_ppo.npz"), **out)


def gen_league():
    """RL/ppo/update_opponent_policies.py: the probability vector for several deque lengths, and the draws of
    update_opponent_policies for a fake rollout manager (numpy global RandomState seeded)."""
    from RL.ppo.update_opponent_policies import get_prob_dist, update_opponent_policies
    out = {}
    sizes = [1, 2, 5, 37, 500, 800, 801, 1000]
    for n in sizes:
        out[f"p_{n}"] = get_prob_dist(n)
    out["sizes"] = np.array(sizes)

    class FakeManager(object):
        def __init__(self, nproc):
            self.processes = list(range(nproc))
            self.calls = []

        def update_policy(self, sd, process_id, policy_id):
            self.calls.append((process_id, policy_id, sd["id"]))

    for (seed, nproc, npol) in [(0, 7, 40), (5, 128, 500), (9, 3, 1)]:
        np.random.seed(seed)
        mgr = FakeManager(nproc)
        update_opponent_policies([{"id": i} for i in range(npol)], mgr, None)
        idx = np.zeros((nproc, 3), dtype=np.int64)
        for (pi, pol, sid) in mgr.calls:
            idx[pi, pol - 1] = sid
        out[f"draw_{seed}_{nproc}_{npol}"] = idx
    np.savez_compressed(os.path.join(OUT, "league.npz"), **out)


def gen_randomise(n_games=6, steps=1800, every=37):
    """Game.randomise_uncertainty (game.py:1207-1282) on states along random games: (blob before, controlling player, blob
    after), generated by the reference with its shuffles routed to the game's philox stream; the game itself continues from
    the un-randomised state (restore_state), as in the forward search."""
    before, after, ctrl_list = [], [], []
    for env_id in range(n_games):
        rng = np.random.default_rng(4242 + env_id)
        ref = rh.RefEnv(21, env_id)
        ref.reset()
        for s in range(steps):
            if s % every == every - 1:
                ctrl = int(rng.integers(1, 5))
                saved, draws = ref.env.save_state(), ref.stream.draws
                before.append(ref.state_blob())
                with rh.patched_rng(ref.stream):
                    ref.env.game.randomise_uncertainty(rh.PIDS[ctrl - 1])
                after.append(ref.state_blob())
                ctrl_list.append(ctrl)
                ref.env.restore_state(saved); ref.stream.draws = draws
            a = rh.random_legal_action(ref.masks(), ref.env, rng)
            _, _, done = ref.step(a)
            if done:
                ref.reset()
    np.savez_compressed(os.path.join(OUT, "randomise.npz"), seed=21, before=np.array(before, dtype=np.int32),
                        after=np.array(after, dtype=np.int32), ctrl=np.array(ctrl_list, dtype=np.int32),
                        env_id=np.repeat(np.arange(n_games), len(before) // n_games).astype(np.int64))
    return len(before)


def _dry_run_game_length(seed, env_id, rng_seed, limit=6000):
    """env steps until the first game of (seed, env_id) ends under the scripted policy seeded with rng_seed"""
    rng = np.random.default_rng(rng_seed)
    e = rh.RefEnv(seed, env_id)
    e.reset()
    for s in range(limit):
        _, _, done = e.step(rh.weighted_legal_action(e.masks(), e.env, rng))
        if done:
            return s + 1
    raise RuntimeError("no game end")


def gen_rollout_small(n_envs=4, T=12, n_rollouts=6, seed=31):
    """SURVEY 8(c) fixture 5: the reference's OWN `GamesAndPoliciesManager.gather_rollouts` / `_after_rollouts`
    (RL/ppo/game_manager.py:69-150) and `BatchProcessor.process_rollouts` (RL/ppo/process_batch.py:37-104) on n_envs games
    x n_rollouts consecutive rollouts of T active-seat decisions, with scripted decisions (ref_harness.ScriptedRefPolicy) and
    every env on its own Philox stream.  Three of the games are advanced (by the same scripted policy, through env.step
    directly) to shortly before their end first, so that game ends, the re-deal, reward / terminal-mask bookkeeping across
    the end and the carry-over into the next rollout are all inside the fixture; the manager's `reset()` then runs with
    `env.reset` disabled so that it adopts those positions.  Stored: the pre-advance actions, every decision of every seat
    during the rollouts (replayed by the collector under test), and the reference's rollout tensors verbatim."""
    import types
    from RL.ppo.game_manager import GamesAndPoliciesManager
    from RL.ppo.process_batch import BatchProcessor
    with rh.patched_rng(rh.PhiloxStream(seed ^ 0xABC, 0)):            # constructor draws (boards, seat orders) from a scratch stream
        mgr = GamesAndPoliciesManager(num_envs=n_envs, num_steps=T)
    rng_seeds = [9000 + i for i in range(n_envs)]
    lengths = [_dry_run_game_length(seed, i, rng_seeds[i]) for i in range(n_envs)]
    pre = [0] + [max(0, lengths[i] - 25 - 30 * i) for i in range(1, n_envs)]   # env 0 starts fresh (initial placement phase)
    streams = [rh.PhiloxStream(seed, i) for i in range(n_envs)]
    ctx = rh.ScriptedContext(mgr.envs, streams, rng_seeds)
    ctx.hook_manager(mgr)
    pol = rh.ScriptedRefPolicy(ctx, mgr.policies[0].lstm_size)
    mgr.policy_maps = [{pid: pol for pid in pm} for pm in mgr.policy_maps]
    pre_actions = []
    for i, env in enumerate(mgr.envs):
        env.reset()
        acts = []
        for _ in range(pre[i]):
            a = rh.weighted_legal_action(env.get_action_masks(), env, ctx.rngs[i])
            _, _, done, _ = env.step(rh.action_to_heads(a))
            assert not done
            acts.append(np.array(a, dtype=np.int8))
        pre_actions.append(np.array(acts, dtype=np.int8).reshape(-1, 18))
    saved = [env.reset for env in mgr.envs]
    for env in mgr.envs:                                              # reset() adopts the current positions
        env.reset = (lambda e: (lambda: e._get_obs()))(env)
    mgr.reset()
    for env, r in zip(mgr.envs, saved):
        env.reset = r
    args = types.SimpleNamespace(num_steps=T, num_processes=1, num_envs_per_process=n_envs, gamma=0.999, gae_lambda=0.95)
    bp = BatchProcessor(args, lstm_dim=mgr.policies[0].lstm_size, device="cpu")
    out = {"seed": seed, "n_envs": n_envs, "T": T, "n_rollouts": n_rollouts,
           "active_pid": np.array([int(p) for p in mgr.active_player_ids], dtype=np.int8),
           "pre_len": np.array(pre, dtype=np.int32), "pre_actions": np.concatenate(pre_actions).astype(np.int8)}
    trace_mark = [0] * n_envs
    for r in range(n_rollouts):
        rollouts = mgr.gather_rollouts()
        mgr._after_rollouts()
        bp.process_rollouts([rollouts])
        for i in range(n_envs):                                       # all-seat decisions taken during this rollout
            seg = np.array(ctx.trace[i][trace_mark[i]:], dtype=np.int8).reshape(-1, 18)
            out[f"r{r}_trace_{i}"] = seg
            trace_mark[i] = len(ctx.trace[i])
        for k in bp.obs_keys:
            v = bp.obs_dict[k].numpy()
            out[f"r{r}_obs_{k}"] = v.astype(np.int8) if v.dtype == np.int64 else v.astype(np.float16)
            assert np.array_equal(out[f"r{r}_obs_{k}"].astype(v.dtype), v), k          # exactly representable
        out[f"r{r}_rewards"] = bp.rewards.numpy()
        out[f"r{r}_masks"] = bp.masks.numpy()
        out[f"r{r}_action_log_probs"] = bp.action_log_probs.numpy()
        for i in range(12):
            out[f"r{r}_actions_{i}"] = bp.actions[i].numpy().astype(np.int8)
            out[f"r{r}_action_masks_{i}"] = bp.action_masks[i].numpy().astype(np.int8)
        out[f"r{r}_games_complete"] = bp.games_complete
        out[f"r{r}_state_crc"] = np.array([crc(rh.state_blob(env, streams[i].draws)) for i, env in enumerate(mgr.envs)], dtype=np.uint32)
    assert bp.games_complete >= 3, bp.games_complete
    # the reference's OWN truncated-BPTT generator (process_batch.py:203-293) on the LAST rollout's tensors, with tagged values /
    # returns / advantages / LSTM states standing in for what compute_advantages_alt and an LSTM net would have left there:
    # the permutation it drew (np.random.permutation, :216) and every tensor of every minibatch tuple, verbatim
    import torch
    L, nmb = 4, 2
    tag = (torch.arange(T + 1)[:, None] * 100.0 + torch.arange(n_envs)[None, :]).float()
    lanes = torch.arange(mgr.policies[0].lstm_size).float() / 1024.0
    bp.values = tag[:, :, None] + 0.5; bp.returns = tag[:T, :, None] + 0.25; bp.advantages = tag[:T, :, None] - 0.75
    bp.hidden_states = (tag[:, :, None] + lanes, -tag[:, :, None] - lanes)
    np.random.seed(5)
    out["lstm_gen_perm"] = np.random.permutation(n_envs * (T // L))
    np.random.seed(5)
    batches = list(bp.generator_lstm(nmb, T * n_envs, L))
    out["lstm_gen_L"], out["lstm_gen_nmb"] = L, nmb
    names9 = ["obs", "hidden", "actions", "action_masks", "value_preds", "returns", "masks", "old_log_probs", "adv"]
    for b, tup in enumerate(batches):
        for name, item in zip(names9, tup):
            if isinstance(item, dict):
                for k, v in item.items():
                    out[f"lstm_gen_b{b}_{name}_{k}"] = v.numpy().astype(np.float32)
            elif isinstance(item, (list, tuple)):
                for i, v in enumerate(item):
                    out[f"lstm_gen_b{b}_{name}_{i}"] = v.numpy().astype(np.float32)
            else:
                out[f"lstm_gen_b{b}_{name}"] = item.numpy().astype(np.float32)
    np.savez_compressed(os.path.join(OUT, "rollout_small.npz"), **out)
    return bp.games_complete, pre, lengths


class _EvalPolicy(object):
    """scripted `act` + the real net's obs / mask / action converters (the evaluation manager calls those on policies[0])"""

    def __init__(self, scripted, real):
        self.s, self.real = scripted, real
        self.lstm_size = real.lstm_size

    def eval(self):
        return self

    def act(self, *a, **kw):
        return self.s.act(*a, **kw)

    def __getattr__(self, name):
        return getattr(self.real, name)


def gen_eval_small(n_games=3, seed=41):
    """The reference's `EvaluationManager.run_evaluation_game` (RL/ppo/evaluation_manager.py:36-74) on n_games full games with
    scripted decisions: the shuffled seat order, (winner, victory points, game steps, policy decisions) and every decision."""
    from RL.ppo.evaluation_manager import EvaluationManager
    out = {"seed": seed, "n_games": n_games}
    for g in range(n_games):
        with rh.patched_rng(rh.PhiloxStream(seed ^ 0xABC, g)):
            mgr = EvaluationManager()
        stream = rh.PhiloxStream(seed, g)
        ctx = rh.ScriptedContext([mgr.env], [stream], [7000 + g])
        ctx.hook_manager(mgr)
        pol = rh.ScriptedRefPolicy(ctx, mgr.policies[0].lstm_size)
        real = mgr.policies
        mgr.policies = [_EvalPolicy(pol, real[0]) for _ in range(4)]
        random.seed(500 + g)                                          # `random.shuffle(self.order)` (evaluation_manager.py:28)
        winner, vps, steps, decisions = mgr.run_evaluation_game()
        out[f"g{g}_order"] = np.array([int(p) for p in mgr.order], dtype=np.int8)
        out[f"g{g}_result"] = np.array([winner, vps, steps, decisions], dtype=np.int32)
        out[f"g{g}_trace"] = np.array(ctx.trace[0], dtype=np.int8)
        out[f"g{g}_final_blob"] = rh.state_blob(mgr.env, stream.draws)
    np.savez_compressed(os.path.join(OUT, "eval_small.npz"), **out)
    return [out[f"g{g}_result"].tolist() for g in range(n_games)]


def _ref_policy_inputs(x):
    """flat fixture inputs -> the reference net's (obs dict, 12-list masks) (RL/models/policy.py:168-191 layouts)"""
    import torch
    B = x["obs_f"].shape[0]
    o = spec.OBS_FLOAT_OFFSETS
    obs = {k: x["obs_f"][:, o[k]:o[k] + int(np.prod(shp))].reshape((B,) + shp).clone() for k, shp in spec.OBS_FLOAT_KEYS.items()}
    for i, k in enumerate(spec.OBS_LIST_KEYS):
        obs[k] = x["lists"][:, i].long()
    masks = []
    for hi, (off, sz, shp) in enumerate(zip(spec.MASK_OFFSETS, spec.MASK_SIZES, spec.MASK_SHAPES)):
        mk = x["masks"][:, off:off + sz].reshape((B,) + shp).clone()
        masks.append(mk.transpose(0, 1).contiguous() if hi in (1, 6, 9) else mk)
    return obs, masks


def _flat_actions(a_r, B):
    import torch
    return torch.cat([torch.stack([t.view(-1) for t in h], 1) if isinstance(h, list) else h.view(B, -1) for h in a_r], 1)


def gen_policy_small(n_games=40, lstm_T=5, lstm_B=8):
    """VERDICT r2 item 2 / SURVEY a21: the reference's OWN net (`build_agent_model()`, RL/models/policy.py:71-111,
    action_heads_module.py:25-312, distributions.py:25-40) with the deterministic weights of tests/policy_fixture.py on real
    observations / masks -> what `act(deterministic)` and `evaluate_actions` return (value, arg-max actions, joint log-prob,
    entropy, incl. the recurrent trade heads) and, for one backward of a weighted sum of them, the norm and a hashed projection
    of every parameter's gradient.  Twice: the default feed-forward net and `include_lstm=True` (one step per row, and the
    T x B truncated-BPTT form with zeros inside the terminal masks)."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib, policy_util, policy_fixture as pf
    from settlers_of_catan_rl_amd.policy import CatanPolicy
    import RL.models.build_agent_model as bam
    out = {}

    def store_inputs(prefix, x):
        f = x["obs_f"].numpy()
        assert np.array_equal(f.astype(np.float16).astype(np.float32), f)
        out[prefix + "obs_f"] = f.astype(np.float16); out[prefix + "lists"] = x["lists"].numpy().astype(np.int8)
        out[prefix + "lens"] = x["lens"].numpy().astype(np.int8)
        out[prefix + "masks"] = np.packbits(x["masks"].numpy().astype(np.uint8), axis=1, bitorder="little")

    def load_fixture_weights(ref, salt):
        sd = ref.state_dict()
        shapes = {k: tuple(v.shape) for k, v in sd.items() if v.numel() > 0 and not k.startswith("value_normaliser.")}
        new = pf.fixture_state_dict(shapes, salt)
        full = dict(sd); full.update(new)
        ref.load_state_dict(full, strict=True)
        names = sorted(shapes)
        return names, np.array([pf.tensor_crc(new[k]) for k in names], dtype=np.uint32)

    def grads_of(ref, names, loss):
        ref.zero_grad()
        loss.backward()
        prm = dict(ref.named_parameters())
        gn = np.array([float(prm[k].grad.double().norm()) if prm[k].grad is not None else 0.0 for k in names])
        gp = np.array([pf.projection(k, prm[k].grad) if prm[k].grad is not None else 0.0 for k in names])
        return gn, gp

    # ---------------- feed-forward net (the reference's default)
    torch.manual_seed(0)
    ref = bam.build_agent_model()
    names, crcs = load_fixture_weights(ref, "ff:")
    ref.eval()
    x = policy_util.oracle_batch_inputs(oracle_lib, n=n_games, seed=8, steps=(0, 7, 60, 300, 700, 1100, 1500, 1900))
    B = x["obs_f"].shape[0]
    store_inputs("ff_", x)
    out["ff_param_names"] = np.array(names); out["ff_param_crc"] = crcs
    obs, masks = _ref_policy_inputs(x)
    cp = lambda d: {k: v.clone() for k, v in d.items()}
    with torch.no_grad():
        v, a, lp, _ = ref.act(cp(obs), None, None, [m.clone() for m in masks], deterministic=True)
        out["ff_act_value"] = v.numpy(); out["ff_act_actions"] = _flat_actions(a, B).numpy().astype(np.int8); out["ff_act_logp"] = lp.numpy()
        # sampled (non-greedy) actions to evaluate: drawn by this package's net on the CPU with the same weights
        mine = CatanPolicy(); mine.load_reference_state_dict(ref.state_dict()); mine.eval()
        # ... with the action TYPE drawn uniformly among each row's legal types, so that the rarely chosen heads (city, robber,
        # steal, development cards, exchange) are evaluated too
        rs = np.random.default_rng(77)
        legal = x["masks"][:, :13].numpy() > 0
        forced = torch.tensor([int(rs.choice(np.flatnonzero(r))) for r in legal])
        _, a_s, _ = mine.act(x["obs_f"], x["lists"], x["lens"], x["masks"], generator=torch.Generator().manual_seed(11),
                             condition_on_action_type=forced)
    out["ff_eval_actions"] = a_s.numpy().astype(np.int8)
    acts_ref = [a_s[:, off:off + ln].clone() for off, ln in spec.ACTION_HEAD_SLICES]
    v, lp, ent, _ = ref.evaluate_actions(cp(obs), None, None, acts_ref, [m.clone() for m in masks])
    out["ff_eval_value"] = v.detach().numpy(); out["ff_eval_logp"] = lp.detach().numpy(); out["ff_eval_entropy"] = float(ent)
    wv, wl = torch.linspace(0.5, 1.5, B)[:, None], torch.linspace(1.5, 0.5, B)[:, None]
    out["ff_grad_norm"], out["ff_grad_proj"] = grads_of(ref, names, (v * wv).sum() + (lp * wl).sum() + 3.0 * ent)
    types = sorted(set(a_s[:, 0].tolist()))

    # ---------------- include_lstm = True (build_agent_model.py:26 switched on)
    old = bam.include_lstm
    bam.include_lstm = True
    try:
        torch.manual_seed(3)
        ref = bam.build_agent_model()
    finally:
        bam.include_lstm = old
    names, crcs = load_fixture_weights(ref, "lstm:")
    ref.eval()
    T, Bs = lstm_T, lstm_B
    x = {k: v[:T * Bs] for k, v in policy_util.oracle_batch_inputs(oracle_lib, n=T * Bs, seed=9, steps=(200,)).items()}
    B = T * Bs
    store_inputs("lstm_", x)
    out["lstm_param_names"] = np.array(names); out["lstm_param_crc"] = crcs; out["lstm_T"] = T; out["lstm_B"] = Bs
    obs, masks = _ref_policy_inputs(x)
    g = torch.Generator().manual_seed(21)
    h0 = torch.randn(B, 256, generator=g) * 0.5; c0 = torch.randn(B, 256, generator=g) * 0.5
    nt = (torch.rand(B, 1, generator=g) > 0.3).float()
    hs = torch.randn(Bs, 256, generator=g) * 0.5; cs = torch.randn(Bs, 256, generator=g) * 0.5
    nts = torch.ones(T, Bs); nts[0, 1] = 0; nts[2, 3] = 0; nts[2, 5] = 0; nts[4, 0] = 0
    nts = nts.reshape(T * Bs, 1)
    for k, t in dict(h0=h0, c0=c0, nt=nt, hs=hs, cs=cs, nts=nts).items():
        out["lstm_" + k] = t.numpy()
    with torch.no_grad():
        v, a, lp, (h1, c1) = ref.act(cp(obs), (h0.clone(), c0.clone()), nt.clone(), [m.clone() for m in masks], deterministic=True)
        out["lstm_act_value"] = v.numpy(); out["lstm_act_actions"] = _flat_actions(a, B).numpy().astype(np.int8)
        out["lstm_act_logp"] = lp.numpy(); out["lstm_act_h"] = h1.numpy(); out["lstm_act_c"] = c1.numpy()
        mine = CatanPolicy(include_lstm=True); mine.load_reference_state_dict(ref.state_dict()); mine.eval()
        _, a_s, _, _ = mine.act(x["obs_f"], x["lists"], x["lens"], x["masks"], generator=torch.Generator().manual_seed(12), hidden=(h0, c0), nonterminal=nt)
    out["lstm_eval_actions"] = a_s.numpy().astype(np.int8)
    acts_ref = [a_s[:, off:off + ln].clone() for off, ln in spec.ACTION_HEAD_SLICES]
    v, lp, ent, (h2, c2) = ref.evaluate_actions(cp(obs), (hs.clone(), cs.clone()), nts.clone(), acts_ref, [m.clone() for m in masks])
    out["lstm_eval_value"] = v.detach().numpy(); out["lstm_eval_logp"] = lp.detach().numpy(); out["lstm_eval_entropy"] = float(ent)
    out["lstm_eval_h"] = h2.detach().numpy(); out["lstm_eval_c"] = c2.detach().numpy()
    wv, wl = torch.linspace(0.5, 1.5, B)[:, None], torch.linspace(1.5, 0.5, B)[:, None]
    out["lstm_grad_norm"], out["lstm_grad_proj"] = grads_of(ref, names, (v * wv).sum() + (lp * wl).sum() + 3.0 * ent)
    np.savez_compressed(os.path.join(OUT, "policy_small.npz"), **out)
    return {"ff_rows": int(out["ff_lens"].shape[0]), "ff_action_types_evaluated": types, "lstm_rows": B,
            "bytes": os.path.getsize(os.path.join(OUT, "policy_small.npz"))}


PPO_UPDATE_ARGS = dict(clip_param=0.2, ppo_epoch=2, num_mini_batch=4, value_loss_coef=1.0, entropy_coef_start=0.04, max_grad_norm=0.5,
                       recompute_returns=True, gamma=0.999, gae_lambda=0.95, lr=3e-4, eps=1e-5, truncated_seq_len=10)
PPO_UPDATE_LRS = (3e-4, 2e-4)          # the second update runs at a lower learning rate (train_loop's linear decay writes param_groups)


def _ref_batch_processor(g, r, dtype):
    """the reference's BatchProcessor holding rollout r of rollout_small.npz (the attributes its process_rollouts wrote, verbatim)"""
    import types
    import torch
    from RL.ppo.process_batch import BatchProcessor, OBS_KEYS
    T, n = int(g["T"]), int(g["n_envs"])
    args = types.SimpleNamespace(num_steps=T, num_processes=1, num_envs_per_process=n, gamma=0.999, gae_lambda=0.95)
    bp = BatchProcessor(args, lstm_dim=256, device="cpu")
    bp.obs_dict = {}
    for k in OBS_KEYS:
        v = g[f"r{r}_obs_{k}"]
        bp.obs_dict[k] = torch.from_numpy(v.astype(np.int64)) if v.dtype == np.int8 else torch.from_numpy(v.astype(np.float32)).to(dtype)
    bp.hidden_states = (torch.zeros(T + 1, n, 256, dtype=dtype), torch.zeros(T + 1, n, 256, dtype=dtype))
    bp.rewards = torch.from_numpy(g[f"r{r}_rewards"]).to(dtype)
    bp.masks = torch.from_numpy(g[f"r{r}_masks"]).to(dtype)
    bp.action_log_probs = torch.from_numpy(g[f"r{r}_action_log_probs"]).to(dtype)
    bp.actions = [torch.from_numpy(g[f"r{r}_actions_{i}"].astype(np.int64)) for i in range(12)]
    bp.action_masks = [torch.from_numpy(g[f"r{r}_action_masks_{i}"].astype(np.float32)).to(dtype) for i in range(12)]
    return bp


def gen_ppo_update(seed=51):
    """VERDICT r6 / the whole-update pin: the reference's OWN `PPO.update` (RL/ppo/ppo.py:25-79: its BatchProcessor's
    compute_advantages_alt and generator_standard, clip_grad_norm_, torch.optim.Adam) on the net `build_agent_model()` with the
    deterministic weights of tests/policy_fixture.py (salt "ppo:", stored as crc32s only), two updates in a row with one optimiser
    (the second at a lower learning rate) on rollouts r0 and r1 of rollout_small.npz (T = 12 x N = 4 = 48 rows, 2 epochs x 4
    minibatches of 12 rows: several action heads have no row in a minibatch).
      - old log-probs: the fixture net's own log-probs of the stored actions + deterministic offsets in about +-0.4 (stored), so
        that the ratios leave [1 - clip, 1 + clip] on both sides in some rows;
      - the samplers' permutations are drawn here (numpy, seeded) and handed to SubsetRandomSampler through torch.randperm;
      - per optimiser step k: the losses ppo.py:77-79 reads (.item() calls of ppo.py), the pre-clip total gradient norm, and per
        parameter whether its gradient is None, whether the step moved it, the gradient's norm and hashed projection
        (policy_fixture.projection), and the norm and projection of theta_k - theta_0.
    Twice: in fp32, and in fp64 (torch's default dtype set to float64 and the net `.double()`: the reference's code then computes
    in fp64 throughout, the BatchProcessor's own torch.zeros included), so that the tests can take their tolerances from the
    reference's own fp32 noise."""
    import torch
    import torch.nn.utils
    import types
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import golden_util as gu
    import policy_fixture as pf
    import RL.models.build_agent_model as bam
    from RL.ppo.ppo import PPO
    g = gu.load("rollout_small.npz")
    T, n = int(g["T"]), int(g["n_envs"])
    rows = T * n
    nmb, epochs, n_upd = PPO_UPDATE_ARGS["num_mini_batch"], PPO_UPDATE_ARGS["ppo_epoch"], len(PPO_UPDATE_LRS)
    rng = np.random.default_rng(seed)
    perms = np.stack([rng.permutation(rows) for _ in range(n_upd * epochs)]).astype(np.int64)          # [update * epoch, rows]
    offsets = (rng.integers(-400, 401, size=(n_upd, T, n)) / 1000.0).astype(np.float32)
    out = {"rollouts": np.array([0, 1], dtype=np.int32), "perms": perms, "lrs": np.array(PPO_UPDATE_LRS),
           "seed": seed}
    for k, v in PPO_UPDATE_ARGS.items():
        out["arg_" + k] = v

    def build(dtype):
        torch.manual_seed(0)
        ref = bam.build_agent_model()
        sd = ref.state_dict()
        shapes = {k: tuple(v.shape) for k, v in sd.items() if v.numel() > 0 and not k.startswith("value_normaliser.")}
        new = pf.fixture_state_dict(shapes, "ppo:")
        full = dict(sd); full.update(new)
        ref.load_state_dict(full, strict=True)
        names = sorted(shapes)
        return ref.to(dtype), names, np.array([pf.tensor_crc(new[k]) for k in names], dtype=np.uint32)

    # the actions: the stored ones, except that the fixture's scripted decisions left the two trade heads' columns at 0 in rows
    # whose action type does not use them, and 0 ("stop") is not a legal FIRST resource of those heads when the player holds
    # resources: the reference evaluates every head on every row and multiplies the masked log-prob by 0, so -inf * 0 = NaN
    # (the reference's own sampler never produces such a row).  Those first entries are replaced by the first legal resource
    # (under the mask RecurrentResourceActionHead.forward forms), the rest by 0.  Then the old log-probs: the fixture net's
    # (fp32) log-probs of those actions at theta_0, + the offsets
    ref, names, crcs = build(torch.float32)
    out["param_names"] = np.array(names); out["param_crc"] = crcs
    for u, r in enumerate(out["rollouts"]):
        bp = _ref_batch_processor(g, int(r), torch.float32)
        obs = {k: v[:-1].reshape((rows,) + tuple(v.shape[2:])) for k, v in bp.obs_dict.items()}
        acts = [a.reshape(rows, -1).clone() for a in bp.actions]
        res = obs["current_resources"]
        for hi in (7, 8):
            head = ref.action_head_module.action_heads[hi]
            mask = (res > 0).float() if head.mask_based_on_curr_res else torch.ones_like(res)
            mask[:, 0] = (res.sum(-1) == 0).float()
            bad = mask.gather(1, acts[hi][:, :1]).view(-1) == 0
            acts[hi][bad] = 0
            acts[hi][bad, 0] = mask[bad].argmax(1)
        masks = [m.reshape(m.shape[0], rows, *m.shape[3:]) if i in (1, 6, 9) else m.reshape(rows, *m.shape[2:]) for i, m in enumerate(bp.action_masks)]
        with torch.no_grad():
            _, lp, _, _ = ref.evaluate_actions(obs, None, bp.masks[:-1].reshape(rows, 1), acts, masks)
        assert bool(torch.isfinite(lp).all()), lp
        out[f"u{u}_actions"] = torch.cat(acts, 1).reshape(T, n, -1).numpy().astype(np.int8)
        out[f"u{u}_old_log_probs"] = (lp.reshape(T, n).numpy() + offsets[u]).astype(np.float32)

    for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        old_default = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            ref, names, _ = build(dtype)
            prm = dict(ref.named_parameters())
            theta0 = {k: prm[k].detach().clone() for k in names}
            agent = PPO(ref, types.SimpleNamespace(**PPO_UPDATE_ARGS))
            rec = {k: [] for k in ("norm", "g_none", "moved", "g_norm", "g_proj", "d_norm", "d_proj")}
            items = []
            clip0, randperm0, item0 = torch.nn.utils.clip_grad_norm_, torch.randperm, torch.Tensor.item
            perm_iter = iter(perms)

            def clip(params, max_norm, *a, **kw):
                rec["g_none"].append([prm[k].grad is None for k in names])
                rec["g_norm"].append([float(prm[k].grad.double().norm()) if prm[k].grad is not None else 0.0 for k in names])
                rec["g_proj"].append([pf.projection(k, prm[k].grad) if prm[k].grad is not None else 0.0 for k in names])
                total = clip0(params, max_norm, *a, **kw)
                rec["norm"].append(float(total))
                return total

            def randperm(m, *a, **kw):
                p = next(perm_iter)
                assert m == len(p)
                return torch.from_numpy(p.copy())

            def item(t):
                v = item0(t)
                if sys._getframe(1).f_code.co_filename.endswith(os.path.join("ppo", "ppo.py")):
                    items.append(v)
                return v

            step0 = agent.optimiser.step

            def step(*a, **kw):
                before = {k: prm[k].detach().clone() for k in names}
                r_ = step0(*a, **kw)
                with torch.no_grad():
                    rec["moved"].append([not torch.equal(before[k], prm[k]) for k in names])
                    d = {k: prm[k].detach() - theta0[k] for k in names}
                rec["d_norm"].append([float(d[k].double().norm()) for k in names])
                rec["d_proj"].append([pf.projection(k, d[k]) for k in names])
                return r_
            agent.optimiser.step = step
            torch.nn.utils.clip_grad_norm_, torch.randperm, torch.Tensor.item = clip, randperm, item
            try:
                returned = []
                for u, r in enumerate(out["rollouts"]):
                    for grp in agent.optimiser.param_groups:
                        grp["lr"] = PPO_UPDATE_LRS[u]
                    bp = _ref_batch_processor(g, int(r), dtype)
                    bp.action_log_probs = torch.from_numpy(out[f"u{u}_old_log_probs"]).to(dtype)[:, :, None]
                    a = torch.from_numpy(out[f"u{u}_actions"].astype(np.int64))
                    bp.actions = [a[:, :, off:off + ln] for off, ln in spec.ACTION_HEAD_SLICES]
                    returned.append(agent.update(bp))
            finally:
                torch.nn.utils.clip_grad_norm_, torch.randperm, torch.Tensor.item = clip0, randperm0, item0
        finally:
            torch.set_default_dtype(old_default)
        n_steps = n_upd * epochs * nmb
        assert len(items) == 3 * n_steps and len(rec["norm"]) == n_steps, (len(items), len(rec["norm"]))
        # ppo.py:77-79 reads value_loss, action_loss, entropy (in that order) and multiplies the first and the last by their coefficients:
        # stored as (value loss x value_loss_coef, action loss, entropy x entropy_coef), the terms update() averages
        coefs = np.array([PPO_UPDATE_ARGS["value_loss_coef"], 1.0, PPO_UPDATE_ARGS["entropy_coef_start"]])
        out[f"{tag}_step_losses"] = np.array(items, dtype=np.float64).reshape(n_steps, 3) * coefs
        out[f"{tag}_update_losses"] = np.array(returned, dtype=np.float64)
        out[f"{tag}_grad_norm_total"] = np.array(rec["norm"], dtype=np.float64)
        out[f"{tag}_grad_none"] = np.packbits(np.array(rec["g_none"], dtype=np.uint8), axis=1, bitorder="little")
        out[f"{tag}_moved"] = np.packbits(np.array(rec["moved"], dtype=np.uint8), axis=1, bitorder="little")
        for k in ("g_norm", "g_proj", "d_norm", "d_proj"):
            out[f"{tag}_{k}"] = np.array(rec[k], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "ppo_update.npz"), **out)
    f32, f64 = out["f32_d_proj"], out["f64_d_proj"]
    scale = np.maximum(out["f64_d_norm"], 1e-3 * out["f64_d_norm"].max(1, keepdims=True))
    return {"bytes": os.path.getsize(os.path.join(OUT, "ppo_update.npz")), "params": len(names),
            "grad_none_f32": int(np.unpackbits(out["f32_grad_none"], axis=1, bitorder="little")[:, :len(names)].sum()),
            "fp32_vs_fp64_dtheta_proj_rel": float((np.abs(f32 - f64) / scale).max()),
            "fp32_vs_fp64_loss_abs": float(np.abs(out["f32_step_losses"] - out["f64_step_losses"]).max()),
            "fp32_vs_fp64_norm_rel": float((np.abs(out["f32_grad_norm_total"] - out["f64_grad_norm_total"]) / out["f64_grad_norm_total"]).max())}


def gen_forward_search(n_ucb_roots=3):
    """the reference's forward-search HOST logic and simulator, as data.
      prop_*   `default_sample_actions` (sample_actions_fn.py:55-329) root by root with the reference net (fixture weights,
               arg-max heads, `random.seed` given): inputs and the proposal lists it returns;
      ucb_*    `_select_action / _update_stats / MovingAvgCalculator` (policy.py:151-177, utils.py) driven with a recorded stream of
               simulation results: every selection it makes, the final choice and the running std;
      sim_*    `run_simulation_forward` + `gae` (worker.py:61-143) from four mid-game states with the same net (arg-max for every
               seat, the game's Philox stream): start blob, searching player, initial action, depth -> value estimate."""
    import copy
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import policy_fixture as pf
    import RL.models.build_agent_model as bam
    from RL.forward_search_policy.sample_actions_fn import default_sample_actions
    from RL.forward_search_policy.policy import ForwardSearchPolicy
    from RL.forward_search_policy.utils import MovingAvgCalculator
    from RL.forward_search_policy.worker import run_simulation_forward
    torch.manual_seed(0)
    ref_net = bam.build_agent_model(device="cpu")
    sd = ref_net.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items() if v.numel() > 0 and not k.startswith("value_normaliser.")}
    full = dict(sd); full.update(pf.fixture_state_dict(shapes, "ff:"))
    ref_net.load_state_dict(full, strict=True)
    ref_net.eval()
    orig = ref_net.act
    ref_net.act = lambda *a, **kw: orig(*a, **{**kw, "deterministic": True})
    out = {}
    # ---- proposals
    F, L, Ln, M, init_flags, seeds, wants = [], [], [], [], [], [], []
    for (seed, warm) in [(3, 0), (3, 5), (3, 60), (3, 300), (6, 700), (6, 1100), (9, 1500), (9, 2100), (12, 2500), (12, 40)]:
        rng = np.random.default_rng(seed + warm)
        ref = rh.RefEnv(seed, 0)
        obs = ref.reset()
        for _ in range(warm):
            obs, _, done = ref.step(rh.random_legal_action(ref.masks(), ref.env, rng))
            if done:
                obs = ref.reset()
        random.seed(1234 + warm)
        masks_t = ref_net.act_masks_to_torch(ref.env.get_action_masks())
        initial = bool(ref.env.game.initial_placement_phase)
        want, _ = default_sample_actions(ref_net.obs_to_torch(copy.deepcopy(obs)), None, masks_t, ref_net, 10, initial_settlement_phase=initial)
        want = np.array([np.concatenate([np.asarray(h).reshape(-1) for h in a]) for a in want], dtype=np.int8)
        f, lists, lens, _ = rh.obs_flat(obs)
        F.append(f); L.append(lists); Ln.append(lens); M.append(rh.masks_flat(ref.masks())); init_flags.append(initial); seeds.append(1234 + warm)
        wants.append(want)
    out["prop_obs_f"] = np.stack(F).astype(np.float16); out["prop_lists"] = np.stack(L).astype(np.int8); out["prop_lens"] = np.stack(Ln).astype(np.int8)
    assert np.array_equal(out["prop_obs_f"].astype(np.float32), np.stack(F))
    out["prop_masks"] = np.packbits(np.stack(M).astype(np.uint8), axis=1, bitorder="little")
    out["prop_initial"] = np.array(init_flags, dtype=np.uint8); out["prop_seed"] = np.array(seeds, dtype=np.int64)
    out["prop_count"] = np.array([len(w) for w in wants], dtype=np.int32)
    out["prop_actions"] = np.concatenate(wants).astype(np.int8)
    # ---- UCB bookkeeping
    rng = np.random.default_rng(1)
    R, A, K = n_ucb_roots, 10, 4
    refs = []
    for r in range(R):
        o = ForwardSearchPolicy.__new__(ForwardSearchPolicy)
        o.value_moving_average = MovingAvgCalculator(window_size=500)
        refs.append(o)
    n_acts, sel, vals_all, best_all, std_all = [], [], [], [], []
    for decision in range(3):
        n_act = rng.integers(2, A + 1, size=R)
        n_acts.append(n_act)
        for r, o in enumerate(refs):
            o.proposed_actions = list(range(n_act[r]))
            o.num_simulations_finished = 0; o.num_simulations_in_progress = 0
            o.num_simulations_finished_each_action = np.zeros(n_act[r]); o.num_simulations_started_each_action = np.zeros(n_act[r])
            o.exploit_scores = np.zeros(n_act[r])
        for rnd in range(40):
            ids = np.zeros((R, K), dtype=np.int64)
            for k in range(K):
                for r, o in enumerate(refs):
                    ar = o._select_action()
                    ids[r, k] = ar
                    o.num_simulations_in_progress += 1; o.num_simulations_started_each_action[ar] += 1
            vals = rng.normal(120, 60, size=(R, K)) + 10 * ids
            for k in range(K):
                for r, o in enumerate(refs):
                    o._update_stats(vals[r, k], ids[r, k])
            sel.append(ids); vals_all.append(vals)
        best_all.append([o._select_action(explore=False) for o in refs])
        std_all.append([o.value_moving_average.get_std() for o in refs])
    out["ucb_n_act"] = np.array(n_acts); out["ucb_sel"] = np.array(sel); out["ucb_vals"] = np.array(vals_all)
    out["ucb_best"] = np.array(best_all); out["ucb_std"] = np.array(std_all, dtype=np.float64)
    # ---- simulations
    blobs, ctrls, inits, depths, values, sim_seeds = [], [], [], [], [], []
    for (seed, warm, depth) in [(5, 40, 6), (5, 400, 8), (8, 900, 5), (11, 1500, 20)]:
        rng = np.random.default_rng(seed)
        ref = rh.RefEnv(seed, 0, dense_reward=True)
        obs = ref.reset()
        for _ in range(warm):
            obs, _, done = ref.step(rh.random_legal_action(ref.masks(), ref.env, rng))
            if done:
                obs = ref.reset()
        blobs.append(ref.state_blob())
        ctrl = ref.deciding_player()
        init = rh.random_legal_action(ref.masks(), ref.env, rng)
        with rh.patched_rng(ref.stream):
            want = run_simulation_forward(ref.env, ref_net, player_id=rh.PIDS[ctrl - 1], init_action=rh.action_to_heads(init), init_player_hs=None,
                                          curr_hidden_states={p: None for p in rh.PIDS}, curr_obs=ref_net.obs_to_torch(copy.deepcopy(obs)),
                                          max_depth=depth, gamma=0.999)
        ctrls.append(ctrl); inits.append(np.asarray(init)); depths.append(depth); values.append(float(want)); sim_seeds.append(seed)
    out["sim_blob"] = np.array(blobs, dtype=np.int32); out["sim_ctrl"] = np.array(ctrls, dtype=np.int32)
    out["sim_init"] = np.array(inits, dtype=np.int8); out["sim_depth"] = np.array(depths, dtype=np.int32)
    out["sim_value"] = np.array(values, dtype=np.float64); out["sim_seed"] = np.array(sim_seeds, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "forward_search.npz"), **out)
    return {"proposal_counts": out["prop_count"].tolist(), "types": sorted(set(out["prop_actions"][:, 0].tolist())), "sim_values": values,
            "bytes": os.path.getsize(os.path.join(OUT, "forward_search.npz"))}


def _in_masks(masks, a):
    """would a policy that samples every head from the reference's masks ever emit `a`? (the head -> mask-row rules of
    RL/models/build_agent_model.py:113-127; heads 6 row 0, 7 and 8 are all ones: the give list is checked against the hand)"""
    m = [np.asarray(x) for x in masks]
    t = int(a[0])
    if not (0 <= t <= 12) or m[0][t] <= 0:
        return False

    def ok(row, i, n):
        return 0 <= int(i) < n and row[int(i)] > 0
    if t == 0: return ok(m[1][0], a[1], 54)
    if t == 2: return ok(m[1][1], a[1], 54)
    if t == 1: return ok(m[2], a[2], 73)
    if t == 8: return ok(m[3], a[3], 19)
    if t == 4:
        if not ok(m[4], a[4], 5): return False
        if a[4] == 4: return ok(m[9][2], a[15], 5)
        if a[4] == 2: return ok(m[9][3], a[15], 5) and ok(m[10], a[16], 5)
        return True
    if t == 5: return ok(m[9][0], a[15], 5) and ok(m[10], a[16], 5)
    if t == 7: return ok(m[5], a[5], 2)
    if t == 11: return ok(m[6][1], a[6], 3)
    if t == 12: return ok(m[11], a[17], 5)
    return True      # types without sub-heads; ProposeTrade's lists are left to the verdict itself


def gen_validate_cases(seed=61, n_states=720, every=31):
    """validate_cases.npz - SURVEY a4: `EnvWrapper.step` with validate_actions=True (the default; env/wrapper.py:36-42) =
    `_translate_action` + `Game.validate_action` (game/game.py:264-525) + `apply_action`.  States are harvested from reference
    games in which some steps are ACCEPTED OUT-OF-MASK actions (so the states only those reach are present); per state a
    set of probe actions (tools/fuzz_validate_vs_ref.py: sampled, random, perturbed, out-of-range, targeted) with the
    reference's verdict and, for every accepted probe, what the reference's state / masks / rewards / done look like after
    it.  Two wrapper configurations: the defaults, and (max_proposed_trades_per_turn=None, max_actions_per_turn=6)."""
    import fuzz_validate_vs_ref as fv
    states, st_trades, st_maxact, st_seed, st_env = [], [], [], [], []
    c_state, c_action, c_accept, c_inmask, c_kind = [], [], [], [], []
    p_crc, p_masks, p_rew64, p_done, p_decide, p_blob_idx, p_blobs = [], [], [], [], [], [], []
    kinds = ["sampled", "random", "perturbed", "out_of_range", "robber_any_tile", "roll_in_road_building", "dummy_edge",
             "propose", "end_turn", "play_owned_card"]
    for cfg_i, (trades, max_actions) in enumerate([(4, None), (None, 6)]):
        for env_id in range(2):
            rng = np.random.default_rng(seed * 1009 + cfg_i * 17 + env_id)
            ref = rh.RefEnv(seed, 10 * cfg_i + env_id, max_proposed_trades_per_turn=trades, max_actions_per_turn=max_actions)
            ref.reset()
            t = 0
            while sum(1 for x in st_env if x == 10 * cfg_i + env_id) < n_states // 4:
                base = rh.random_legal_action(ref.masks(), ref.env, rng)
                probes = fv.probes_for(rng, base, 4, ref)
                verdicts = [fv.ref_verdict(ref, a) for _, a in probes]
                masks_now = ref.masks()
                # kept: states right after an out-of-mask step, states with an accepted out-of-mask probe, and every `every`-th one
                has_exotic = any(v and not _in_masks(masks_now, a) for (_, a), v in zip(probes, verdicts))
                if t % every == 0 or getattr(ref, "_exotic", False) or has_exotic:
                    si = len(states)
                    blob = ref.state_blob()
                    states.append(blob); st_trades.append(-1 if trades is None else trades)
                    st_maxact.append(-1 if max_actions is None else max_actions); st_seed.append(seed); st_env.append(10 * cfg_i + env_id)
                    for (kind, a), v in zip(probes, verdicts):
                        c_state.append(si); c_action.append(a.astype(np.int32)); c_accept.append(int(v))
                        c_inmask.append(int(_in_masks(masks_now, a) and (v or int(a[0]) != 6))); c_kind.append(kinds.index(kind))   # ProposeTrade: the give list must be owned
                        if v:
                            cp = ref.clone()
                            _, rew, done = cp.step(a)
                            pb = cp.state_blob()
                            p_crc.append(crc(pb)); p_masks.append(pack_masks(rh.masks_flat(cp.masks())))
                            p_rew64.append(cp.last_reward64.copy()); p_done.append(int(done)); p_decide.append(cp.deciding_player())
                            if not c_inmask[-1]:
                                p_blob_idx.append(len(c_state) - 1); p_blobs.append(pb)
                            assert np.array_equal(ref.state_blob(), blob)
                        else:
                            p_crc.append(0); p_masks.append(np.zeros(41, dtype=np.uint8)); p_rew64.append(np.zeros(4)); p_done.append(0); p_decide.append(0)
                # the game's real step: now and then an accepted action from outside the masks
                exotic = [a for (k, a), v in zip(probes, verdicts) if v and not _in_masks(masks_now, a)]
                ref._exotic = False
                a = base
                if exotic and rng.random() < 0.35:
                    a = exotic[int(rng.integers(0, len(exotic)))]
                    ref._exotic = True
                _, _, done = ref.step(a)
                if done:
                    ref.reset()
                t += 1
    c_accept = np.array(c_accept, dtype=np.uint8); c_inmask = np.array(c_inmask, dtype=np.uint8)
    assert not (c_inmask & (1 - c_accept)).any(), "an in-mask action the reference rejects"
    np.savez_compressed(
        os.path.join(OUT, "validate_cases.npz"), kinds=np.array(kinds),
        states=np.array(states, dtype=np.int16), state_trades=np.array(st_trades, dtype=np.int8), state_max_actions=np.array(st_maxact, dtype=np.int8),
        state_seed=np.array(st_seed, dtype=np.int32), state_env=np.array(st_env, dtype=np.int32),
        case_state=np.array(c_state, dtype=np.int32), case_action=np.array(c_action, dtype=np.int32), case_accept=c_accept,
        case_in_masks=c_inmask, case_kind=np.array(c_kind, dtype=np.uint8),
        post_crc=np.array(p_crc, dtype=np.uint32), post_masks=np.array(p_masks, dtype=np.uint8), post_reward64=np.array(p_rew64, dtype=np.float64),
        post_done=np.array(p_done, dtype=np.uint8), post_deciding=np.array(p_decide, dtype=np.int8),
        post_blob_case=np.array(p_blob_idx, dtype=np.int32), post_blobs=np.array(p_blobs, dtype=np.int16))
    oom = (c_accept == 1) & (c_inmask == 0)
    ca = np.array(c_action)
    return dict(states=len(states), cases=len(c_state), accepted=int(c_accept.sum()), accepted_out_of_mask=int(oom.sum()),
                out_of_mask_by_type={int(t): int(((ca[:, 0] == t) & oom).sum()) for t in range(13) if ((ca[:, 0] == t) & oom).any()})


def gen_ref_checks():
    """ref_checks.npz: what the reference returned in the checks that used to import it at test time.
      eval_*      EvaluationManager.run_evaluation_game (evaluation_manager.py) with a scripted uniform-random legal policy keyed by
                  (game, decision number) on the philox game streams: seat orders and (winner, policy-0 VPs, game length, policy-0
                  decisions) of 4 games (tests/test_evaluation_cpu.py)
      bptt_*      BatchProcessor.generator_lstm (process_batch.py:203-293) on a tagged storage: every field of every minibatch
      vre_*       compute_advantages_alt (process_batch.py:112-128) with an LSTM stand-in net: its inputs, the rows it evaluated and
                  the values it stored (tests/test_lstm_bptt_cpu.py)
      sd_*        the names and shapes of build_agent_model().state_dict(), the key set a strict load_state_dict checks
                  (tests/test_policy.py)"""
    import types
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    out = {}
    # ---------------- evaluation episodes
    from RL.ppo.evaluation_manager import EvaluationManager
    import ctypes as C
    seed, n = 31, 4

    def scripted(L, env_ptr, env_id, step, masks_flat):
        m = np.ascontiguousarray(masks_flat, dtype=np.float32)
        a = np.zeros(18, dtype=np.int32)
        L.orc_sample_action(env_ptr, seed + 99, env_id, int(step), m.ctypes.data_as(C.POINTER(C.c_float)), a.ctypes.data_as(C.POINTER(C.c_int32)))
        return a

    class EnvAdapter(object):
        def __init__(self, env_id):
            self.r = rh.RefEnv(seed, env_id)
            self.env_id, self.steps = env_id, 0
            self.mirror = oracle_lib.OracleEnv(seed, env_id)        # supplies the scripted policy with its hand-dependent draws

        @property
        def game(self): return self.r.env.game

        @property
        def winner(self): return self.r.env.winner

        @property
        def curr_vps(self): return self.r.env.curr_vps

        def reset(self):
            self.mirror.reset()
            return self.r.reset()

        def get_action_masks(self):
            return self.r.env.get_action_masks()

        def step(self, a):
            flat = np.concatenate([np.asarray(h).reshape(-1) for h in a]).astype(np.int32)
            with rh.patched_rng(self.r.stream):
                res = self.r.env.step(a)
            self.mirror.step(flat)
            self.steps += 1
            return res

    class FakePolicy(object):
        lstm_size = 4
        dummy_param = torch.empty(1)

        def __init__(self, mgr): self.mgr = mgr
        def eval(self): pass
        def obs_to_torch(self, obs): return obs
        def act_masks_to_torch(self, masks): return masks
        def torch_act_to_np(self, a): return a

        def act(self, obs, hs, tm, masks, deterministic=False):
            ad = self.mgr.env
            a = scripted(ad.mirror.L, ad.mirror.p, ad.env_id, ad.steps, rh.masks_flat(masks))
            return None, rh.action_to_heads(a), None, hs

    mgr = EvaluationManager.__new__(EvaluationManager)
    mgr.policies = [FakePolicy(mgr) for _ in range(4)]
    mgr.device = torch.device("cpu")
    want, orders = [], []
    random.seed(77)
    for g in range(n):
        mgr.env = EnvAdapter(g)
        want.append([int(x) for x in mgr.run_evaluation_game()])
        orders.append([int(p) for p in mgr.order])
        assert np.array_equal(mgr.env.r.state_blob(), mgr.env.mirror.export())
    out.update(eval_seed=np.int64(seed), eval_orders=np.array(orders, dtype=np.int64), eval_want=np.array(want, dtype=np.int64))
    # ---------------- truncated-BPTT minibatches
    from RL.ppo.process_batch import BatchProcessor
    T, N, L, nmb, H = 20, 6, 5, 4, 3
    args = types.SimpleNamespace(num_steps=T, num_processes=N, num_envs_per_process=1, gamma=0.99, gae_lambda=0.95)
    bp = BatchProcessor(args, H, obs_keys=["a", "b"], obs_type=["normal", "normal"], num_action_heads=3,
                        type_conditional_masks=[1], device="cpu")
    gen = torch.Generator().manual_seed(0)
    tag = (torch.arange(T + 1)[:, None] * 100 + torch.arange(N)[None, :]).float()          # value = 100 t + game
    bp.obs_dict = {"a": tag[:, :, None] + torch.tensor([0.0, 0.25]), "b": tag[:, :, None] * 2}
    bp.hidden_states = (tag[:, :, None] + torch.tensor([0.1, 0.2, 0.3]), -tag[:, :, None] - torch.tensor([0.1, 0.2, 0.3]))
    bp.actions = [tag[:T, :, None].long() + i for i in range(3)]
    bp.action_masks = [tag[:T, :, None] + 0.5, torch.stack([tag[:T, :, None] + 1, tag[:T, :, None] + 2]), tag[:T, :, None] + 3]
    bp.values = tag[:, :, None] + 7; bp.returns = tag[:T, :, None] + 8
    bp.masks = (torch.rand(T + 1, N, 1, generator=gen) > 0.2).float()
    bp.action_log_probs = tag[:T, :, None] + 9; bp.advantages = tag[:T, :, None] + 10
    np.random.seed(5)
    batches = list(bp.generator_lstm(nmb, T * N, L))
    out["bptt_masks"] = bp.masks.numpy()
    fields = {"obs_a": lambda b: b[0]["a"], "obs_b": lambda b: b[0]["b"], "hid0": lambda b: b[1][0], "hid1": lambda b: b[1][1],
              "act0": lambda b: b[2][0], "act1": lambda b: b[2][1], "act2": lambda b: b[2][2], "amask0": lambda b: b[3][0],
              "amask1": lambda b: b[3][1], "vpred": lambda b: b[4], "ret": lambda b: b[5], "msk": lambda b: b[6],
              "oldlp": lambda b: b[7], "adv": lambda b: b[8]}
    for k, f in fields.items():
        out["bptt_" + k] = np.stack([f(b).numpy() for b in batches])
    # ---------------- the LSTM value re-evaluation rule
    T, N, H = 4, 3, 2
    args = types.SimpleNamespace(num_steps=T, num_processes=N, num_envs_per_process=1, gamma=0.9, gae_lambda=0.8)
    bp = BatchProcessor(args, H, obs_keys=["a"], obs_type=["normal"], device="cpu")
    gen = torch.Generator().manual_seed(1)
    bp.obs_dict = {"a": torch.randn(T + 1, N, 2, generator=gen)}
    bp.hidden_states = (torch.randn(T + 1, N, H, generator=gen), torch.randn(T + 1, N, H, generator=gen))
    bp.masks = (torch.rand(T + 1, N, 1, generator=gen) > 0.3).float()
    bp.rewards = torch.randn(T, N, 1, generator=gen)
    seen = []

    class Net(object):
        include_lstm, use_value_normalisation = True, False
        def get_value(self, obs, hidden, masks):
            seen.append((obs["a"].clone(), hidden[0].clone(), hidden[1].clone(), masks.clone()))
            return (obs["a"].sum(1, keepdim=True) + (hidden[0] * masks).sum(1, keepdim=True))
    bp.compute_advantages_alt(Net(), max_processes_at_once=2)
    out.update(vre_obs=bp.obs_dict["a"].numpy(), vre_h=bp.hidden_states[0].numpy(), vre_c=bp.hidden_states[1].numpy(),
               vre_masks=bp.masks.numpy(), vre_values=bp.values.numpy(),
               vre_call_rows=np.array([s[0].shape[0] for s in seen], dtype=np.int64),
               vre_call_obs=np.concatenate([s[0].numpy() for s in seen]), vre_call_h=np.concatenate([s[1].numpy() for s in seen]),
               vre_call_c=np.concatenate([s[2].numpy() for s in seen]), vre_call_masks=np.concatenate([s[3].numpy() for s in seen]))
    # ---------------- the reference net's state-dict layout
    from RL.models.build_agent_model import build_agent_model
    sd = build_agent_model().state_dict()
    names = sorted(sd)
    out["sd_names"] = np.array(names)
    out["sd_shapes"] = np.array([list(sd[k].shape) + [-1] * (4 - sd[k].dim()) for k in names], dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "ref_checks.npz"), **out)
    return {k: v.shape for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# Rule-case trajectories: branches of the rules that no random-policy trajectory above reaches.  The reference cannot import
# a state, so every case is a game played from reset: the CPU oracle SCOUTS (it plays the first games of consecutive env ids
# with the device's random policy, orc_sample_action, and the cases are recognised in its consecutive state blobs), the
# reference JUDGES (gen_traj replays the chosen action list; everything stored is what the reference produced).
RULE_SEED, RULE_GAMES = 23, 8192
RULE_CASES = ["lr_takeover", "lr_tie_keep", "lr_tie_vacate", "lr_none_vacate", "lr_takeover_order", "lr_takeover_after_tie", "rb_dummy_edge",
              "yop_bank_short", "city_none_left"]
RULE_TAIL = 48              # steps replayed after the event (after the title is claimed again, for the two vacate cases)
_M = dict(zip(range(12), spec.MASK_OFFSETS))


def _scout_game(env_id, seed=RULE_SEED, limit=6000):
    """-> (env_id, game length, [(case, step)], [(step, lr_player after it)] where the title changed hands).  One deviation from
    the random policy: whenever Year of Plenty is playable while the bank lacks a resource, it is played with that resource as
    the first pick (no mask offers that pick; validate_action accepts it, game.py:403-408, and apply_action skips it, :684-689)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib
    f = spec.state_field
    e = oracle_lib.OracleEnv(seed, env_id)
    e.reset()
    prev = e.export()
    events, title, actions = [], [], []
    for t in range(limit):
        m = e.masks()
        a = e.sample_action(seed, env_id, t, m)
        p = int(f(prev, "players_go")[0])
        bank = f(prev, "bank_res")
        if m[4] > 0 and m[_M[4] + 2] > 0 and (bank == 0).any():                           # Year of Plenty (card 2) with a short bank
            a[:] = 0
            a[0], a[4], a[15], a[16] = 4, 2, int(np.flatnonzero(bank == 0)[0]), int(np.flatnonzero(bank > 0)[0])
            assert m[_M[10] + a[15]] == 0 and m[_M[9] + 10 + a[15]] == 0       # wrapper.py:267-269
            events.append(("yop_bank_short", t))
        if m[1] > 0 and m[_M[2] + 72] > 0:                                    # road building, no legal edge
            events.append(("rb_dummy_edge", t))
        if m[10] > 0 and m[2] == 0:                                           # own turn after the roll (EndTurn offered), no city offered
            res = f(prev, f"p{p}_res")
            own = ((f(prev, "corner_bld") == 1) & (f(prev, "corner_owner") == p)).any()
            if res[4] >= 2 and res[2] >= 3 and f(prev, "cities_left")[p - 1] == 0 and own:
                events.append(("city_none_left", t))
        actions.append(a.copy())
        _, done = e.step(a)
        cur = e.export()
        h, h2 = int(f(prev, "lr_player")[0]), int(f(cur, "lr_player")[0])
        if h != h2:
            title.append((t, h2))
        if a[0] == 0 and h and not f(prev, "initial_phase")[0]:               # a settlement: the only action that shortens a road
            eo, co = f(cur, "edge_owner"), f(cur, "corner_owner")
            ln = {q: oracle_lib.longest_path_raw(eo, co, q) for q in (1, 2, 3, 4)}
            # (update_longest_road stores only the holder's new length: kept are the cuts after which every player's stored
            #  current_longest_path is the true one, so that the tests can read the case off the reference's blobs alone)
            stored = all(ln[q] == int(f(cur, "cur_longest_path")[q - 1]) for q in (1, 2, 3, 4))
            if ln[h] < int(f(prev, "lr_count")[0]) and stored:                # the holder's road was cut
                others = [ln[q] for q in (1, 2, 3, 4) if q != h]
                if h2 not in (0, h):
                    events.append(("lr_takeover_order" if sum(x > ln[h] for x in others) >= 2 else "lr_takeover", t))
                    order = [q for q in (1, 2, 3, 4) if q != h]                # game.py:886
                    if any(ln[o] == ln[h] for o in order[:order.index(h2)]):  # the loop met a tie with the holder before it met the winner
                        events.append(("lr_takeover_after_tie", t))
                elif h2 == 0:
                    events.append(("lr_tie_vacate" if max(others) >= 5 else "lr_none_vacate", t))
                elif ln[h] >= 5 and ln[h] in others:
                    events.append(("lr_tie_keep", t))
        if done:
            break
        prev = cur
    return env_id, len(actions), events, title, actions


def _scout_summary(env_id):
    r = _scout_game(env_id)
    return r[:4]


def scout_rule_cases(n_games=RULE_GAMES, workers=8):
    """-> {case: (env_id, event step, number of steps to replay, step at which the vacant title is claimed again or -1)}: per case the occurrence with the smallest step index whose
    tail (RULE_TAIL steps; for the vacate cases RULE_TAIL steps after somebody claims the title again, game.py:874-878) lies
    inside the game, and how many of the scouted games hold the case at all."""
    import multiprocessing as mp
    with mp.Pool(workers) as pool:
        games = pool.map(_scout_summary, range(n_games), chunksize=32)
    best, count = {}, {c: 0 for c in RULE_CASES}
    for env_id, length, events, title in games:
        for case in set(c for c, _ in events):
            count[case] += 1
        for case, step in events:
            end, claim = step + 1 + RULE_TAIL, -1
            if case in ("lr_tie_vacate", "lr_none_vacate"):
                claimed = [t for t, who in title if t > step and who != 0]
                if not claimed:
                    continue
                claim = claimed[0]
                end = claim + 1 + RULE_TAIL
            if end > length:                 # the whole tail lies inside the first game
                continue
            if case not in best or (step, env_id) < (best[case][1], best[case][0]):
                best[case] = (env_id, step, end, claim)
    return best, count


def gen_rule_trajs(picks=None):
    """tests/golden/traj_rule_<case>.npz: the reference's replay of the scouted action lists (`event`, `event_step` stored besides
    the fields of every trajectory, and `claim_step`: the step at which the vacant title is claimed again, -1 elsewhere; blob and
    observation forced at the event step, the steps around it and the claim).  As generated: seed 23, the first games of env ids
    0..8191 scouted, every case found (`games` = how many of the 8 192 games hold it); the earliest occurrence is taken:

      case                    env id  event step  steps  games  what happens at the event step
      lr_takeover               5393         364    413    114  a settlement cuts the holder's road, ONE other player is longer: title moves
      lr_tie_keep               4118         540    589     83  cut, another player level with the holder at >= 5: holder keeps it, smaller count
      lr_tie_vacate              209         872    927     14  cut, two others level above the holder: title vacated, nobody gains (claimed at 878)
      lr_none_vacate            6726         266    466     21  cut, nobody has 5 left: title vacated (claimed again at 417)
      lr_takeover_order         3024         487    536     23  cut, TWO others longer than the holder: the longest takes the title
      lr_takeover_after_tie      666         514    563     15  cut, the loop of game.py:886 meets a player level with the holder, then the winner
      rb_dummy_edge              462         792    841    258  road building with no legal edge: only edge 72 offered, nothing placed
      yop_bank_short            2482         184    233     76  Year of Plenty, bank short of a resource: mask bit 0, the forced pick is skipped
      city_none_left            8119         664    713     37  wheat >= 2, ore >= 3, a settlement, no city piece left: no city offered

    lr_takeover_after_tie is the one case in which dropping the `tied = False` of game.py:894 changes
    the outcome.  The order of game.py:886 itself cannot change an outcome (the loop computes the maximum and whether two players
    share it, both independent of the order), so no fixture can tell a permuted loop from the reference's.
    """
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    if picks is None:
        picks, count = scout_rule_cases()
        print("games holding each case:", count)
    out = {}
    for case in RULE_CASES:
        if case not in picks:
            print(case, "NOT FOUND in", RULE_GAMES, "games")
            continue
        env_id, step, end, claim = picks[case]
        actions = _scout_game(env_id)[4][:end]
        games = gen_traj(RULE_SEED, env_id, len(actions), name=f"traj_rule_{case}.npz", actions=actions,
                         also_sample=[s for s in (step - 1, step, step + 1, step + 2, claim, claim + 1) if 0 <= s < len(actions)],
                         extra=dict(event=np.array(case), event_step=np.int32(step), claim_step=np.int32(claim)))
        out[case] = dict(env_id=env_id, event_step=step, steps=len(actions), games_finished=games,
                         bytes=os.path.getsize(os.path.join(OUT, f"traj_rule_{case}.npz")))
        print(case, out[case])
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "rule_scout":
        print(scout_rule_cases()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "rule_cases":
        gen_rule_trajs(); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "rollout":
        print("rollout_small (games complete, pre-advance, first-game lengths):", gen_rollout_small()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "eval":
        print("eval_small (winner, vps, steps, decisions):", gen_eval_small()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "randomise":
        print("randomise", gen_randomise()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "kwargs":
        print("dense x 0.37, 1 trade/turn: games", gen_traj(5, 2, 2400, name="traj_dense037_t1_s5_e2.npz", dense=True, anneal=0.37, trades=1))
        print("dense, unlimited trades: games", gen_traj(5, 3, 2400, name="traj_dense_tnone_s5_e3.npz", dense=True, anneal=1.0, trades=None))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "maxact":
        print("max_actions_per_turn = 2: games", gen_traj(7, 1, 5200, name="traj_maxact2_s7_e1.npz", max_actions=2))
        sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "forward_search":
        print("forward_search", gen_forward_search()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "policy":
        print("policy_small", gen_policy_small()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "ppo_update":
        print("ppo_update", gen_ppo_update()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "gae_ppo":
        gen_gae_ppo(); print("gae/ppo"); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "validate":
        print("validate_cases", gen_validate_cases()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "ref_checks":
        print("ref_checks", gen_ref_checks()); sys.exit(0)
    if len(sys.argv) > 1 and sys.argv[1] == "league":
        gen_league(); print("league"); sys.exit(0)
    gen_topology(); print("topology")
    gen_resets(); print("resets")
    for (s, eid, steps) in [(3, 0, 2600), (3, 1, 2600), (17, 4, 1800)]:
        print("traj", s, eid, "games", gen_traj(s, eid, steps))
    gen_mt_kat(); print("mt kat")
    gen_longest_road(); print("longest road")
    gen_gae_ppo(); print("gae/ppo")
    gen_league(); print("league")
    print("randomise", gen_randomise())
    print("dense x 0.37, 1 trade/turn: games", gen_traj(5, 2, 2400, name="traj_dense037_t1_s5_e2.npz", dense=True, anneal=0.37, trades=1))
    print("dense, unlimited trades: games", gen_traj(5, 3, 2400, name="traj_dense_tnone_s5_e3.npz", dense=True, anneal=1.0, trades=None))
    print("max_actions_per_turn = 2: games", gen_traj(7, 1, 5200, name="traj_maxact2_s7_e1.npz", max_actions=2))
    print("rollout_small", gen_rollout_small())
    print("eval_small", gen_eval_small())
    print("policy_small", gen_policy_small())
    print("forward_search", gen_forward_search())
    print("validate_cases", gen_validate_cases())
    print("ref_checks", gen_ref_checks())
    print("rule cases", gen_rule_trajs())
    os.system(f"ls -la {OUT}; du -sh {OUT}")
