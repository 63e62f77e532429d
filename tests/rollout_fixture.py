"""Replays of the fixtures the reference's own managers produced (tools/gen_golden.py `gen_rollout_small`, `gen_eval_small`):
shared by the CPU tests (oracle-backed stand-in env) and the `-m gpu` tests (HIP env)."""
import numpy as np
import torch

import golden_util as gu
from settlers_of_catan_rl_amd import spec


class CountingEnv(object):
    """Delegates to a batched env and counts the real (non no-op) steps of every game."""

    def __init__(self, env):
        self.env, self.n, self.device = env, env.n, env.device
        self.steps_taken = torch.zeros(env.n, dtype=torch.long)

    def step(self, actions):
        self.steps_taken += (actions[:, 0] >= 0).cpu().long()
        return self.env.step(actions)

    def step_deferred(self, actions, window=32, status_out=None):
        """a waiting game's action is ignored by the env: not a step of that game"""
        waiting = getattr(self, "_waiting", None)
        took = (actions[:, 0] >= 0).cpu()
        if waiting is not None:
            took &= ~waiting
        self.steps_taken += took.long()
        r, d, s = self.env.step_deferred(actions, window, status_out=status_out)
        self._waiting = (s == 1).cpu()
        return r, d, s

    def step_flush(self):
        self._waiting = None
        return self.env.step_flush()

    def __getattr__(self, name):
        return getattr(self.env, name)


def scripted_log_prob(a):
    return -0.25 - (a.sum(-1) % 7).float()


class ReplayPolicy(object):
    """Every game takes the recorded decision number `steps_taken[game]` of its trace (all seats)."""
    include_lstm = False

    def __init__(self, cenv, traces):
        self.cenv = cenv
        L = max(len(t) for t in traces)
        self.table = torch.zeros((cenv.n, L + 1, spec.ACTION_WORDS), dtype=torch.int64)
        for i, t in enumerate(traces):
            self.table[i, :len(t)] = torch.from_numpy(np.asarray(t)).long()
        self.lens = torch.tensor([len(t) for t in traces])

    def to(self, *_a, **_k):
        return self

    def eval(self):
        return self

    def load_reference_state_dict(self, sd):
        pass

    wants_games = True      # (the collector may evaluate a list of games instead of all of them: row j = game games[j])

    def act(self, f, lists, lens, masks, generator=None, deterministic=False, games=None, **_kw):
        k = torch.minimum(self.cenv.steps_taken, self.lens)
        a = self.table[torch.arange(self.cenv.n), k]
        if games is not None:
            a = a[games.cpu().long()]
        a = a.to(f.device)
        return torch.zeros(a.shape[0], 1, device=f.device), a, scripted_log_prob(a)[:, None].to(f.device)


def pre_advance(env, pre_len, pre_actions):
    """games are advanced by their recorded pre-advance actions (different lengths: the others idle with no-ops)"""
    n = env.n
    offs = np.concatenate([[0], np.cumsum(pre_len)])
    for s in range(int(max(pre_len)) if n else 0):
        a = torch.full((n, spec.ACTION_WORDS), 0, dtype=torch.int32)
        for i in range(n):
            if s < pre_len[i]:
                a[i] = torch.from_numpy(pre_actions[offs[i] + s].astype(np.int32))
            else:
                a[i, 0] = -1
        _, done = env.step(a.to(env.device))
        assert not bool(done.any())


def check_rollout_fixture(make_env, collector_kwargs=None, on_rollout=None):
    """make_env(n, seed) -> freshly created batched env with auto-reset.  Drives `reference_api.SubProcGameManager` +
    `BatchProcessor` over it and compares every rollout with the tensors of the reference's GamesAndPoliciesManager +
    BatchProcessor (verbatim layouts); on_rollout(r, batch processor, rollouts handle), if given, sees every rollout after its
    checks.  Returns (manager, batch processor, last rollouts handle)."""
    import types
    from settlers_of_catan_rl_amd import reference_api as ra
    g = gu.load("rollout_small.npz")
    n, T, R, seed = int(g["n_envs"]), int(g["T"]), int(g["n_rollouts"]), int(g["seed"])
    env = make_env(n, seed)
    pre_advance(env, g["pre_len"], g["pre_actions"])
    cenv = CountingEnv(env)
    traces = [np.concatenate([g[f"r{r}_trace_{i}"] for r in range(R)]) for i in range(n)]
    mgr = ra.SubProcGameManager([ra.make_game_manager(n, T)], env_factory=lambda n_: cenv,
                                make_policy=lambda: ReplayPolicy(cenv, traces), self_play=True, autocast_dtype=None, collector_kwargs=collector_kwargs)
    col = mgr.collector
    col.active_pid[:] = torch.from_numpy(g["active_pid"].astype(np.int64)).to(col.active_pid.device)
    col.reset()                                           # game_manager.py:35-59 on the adopted positions
    args = types.SimpleNamespace(num_steps=T, num_processes=1, num_envs_per_process=n, gamma=0.999, gae_lambda=0.95)
    bp = ra.BatchProcessor(args, lstm_dim=256, device=env.device)
    ends = 0
    for r in range(R):
        ro = mgr.gather_rollouts()
        bp.process_rollouts(ro)
        for k in ra.OBS_KEYS:
            want = g[f"r{r}_obs_{k}"]
            got = bp.obs_dict[k].cpu().numpy()
            assert got.shape == want.shape, (r, k, got.shape, want.shape)
            assert np.array_equal(got.astype(np.float64), want.astype(np.float64)), (r, k)
        assert bp.rewards.shape == (T, n, 1) and np.array_equal(bp.rewards.cpu().numpy(), g[f"r{r}_rewards"]), r
        assert bp.masks.shape == (T + 1, n, 1) and np.array_equal(bp.masks.cpu().numpy(), g[f"r{r}_masks"]), r
        assert np.array_equal(bp.action_log_probs.cpu().numpy(), g[f"r{r}_action_log_probs"]), r
        for i in range(12):
            assert np.array_equal(bp.actions[i].cpu().numpy(), g[f"r{r}_actions_{i}"].astype(np.int64)), (r, i)
            want = g[f"r{r}_action_masks_{i}"].astype(np.float32)
            got = bp.action_masks[i].cpu().numpy()
            assert got.shape == want.shape and np.array_equal(got, want), (r, i, got.shape, want.shape)
        assert bp.games_complete == int(g[f"r{r}_games_complete"]), r
        blobs = env.export_state().cpu().numpy()
        assert [gu.crc(b) for b in blobs] == [int(c) for c in g[f"r{r}_state_crc"]], r
        ends += int((g[f"r{r}_masks"] == 0).sum())
        if on_rollout is not None:
            on_rollout(r, bp, ro)
    assert ends >= 3                                       # the fixture covers game ends and the carry-over behind them
    check_generator_lstm(g, bp, T, n)
    return mgr, bp, ro


def check_generator_lstm(g, bp, T, n):
    """`BatchProcessor.generator_lstm` (process_batch.py:203-293) on the last rollout: the reference's generator ran on the same
    tensors with tagged values / returns / advantages / LSTM states and the stored permutation; every tensor of every
    minibatch tuple must be the reference's (shapes included: time-major rows, (n, lstm) states, (types, rows, d) masks)."""
    st = bp.storage
    dev = st.obs_f.device
    L, nmb = int(g["lstm_gen_L"]), int(g["lstm_gen_nmb"])
    tag = (torch.arange(T + 1)[:, None] * 100.0 + torch.arange(n)[None, :]).float().to(dev)
    lanes = (torch.arange(256).float() / 1024.0).to(dev)
    bp._values = tag + 0.5; bp._returns = tag[:T] + 0.25; bp._adv = tag[:T] - 0.75
    st.hidden = torch.stack((tag[:, :, None] + lanes, -tag[:, :, None] - lanes))
    bp._cache.pop("hidden", None)
    bp._permutation = lambda count, device: torch.from_numpy(g["lstm_gen_perm"].astype(np.int64)).to(device)
    names9 = ["obs", "hidden", "actions", "action_masks", "value_preds", "returns", "masks", "old_log_probs", "adv"]
    batches = list(bp.generator_lstm(nmb, T * n, L))
    assert len(batches) == nmb
    for b, tup in enumerate(batches):
        assert len(tup) == 9
        for name, item in zip(names9, tup):
            if isinstance(item, dict):
                pairs = [(f"lstm_gen_b{b}_{name}_{k}", v) for k, v in item.items()]
            elif isinstance(item, (list, tuple)):
                pairs = [(f"lstm_gen_b{b}_{name}_{i}", v) for i, v in enumerate(item)]
            else:
                pairs = [(f"lstm_gen_b{b}_{name}", item)]
            for key, v in pairs:
                want = g[key]
                got = v.float().cpu().numpy()
                assert got.shape == want.shape, (key, got.shape, want.shape)
                assert np.array_equal(got, want), key
    st.hidden = None
    bp._cache.pop("hidden", None)


def check_eval_fixture(make_env):
    """make_env(n, seed) -> freshly created env WITHOUT auto-reset: `evaluation.run_evaluation_episodes` against the
    reference's EvaluationManager.run_evaluation_game (winner index, victory points, game length, policy decisions)."""
    from settlers_of_catan_rl_amd import evaluation
    g = gu.load("eval_small.npz")
    n, seed = int(g["n_games"]), int(g["seed"])
    env = make_env(n, seed)
    cenv = CountingEnv(env)
    traces = [g[f"g{i}_trace"] for i in range(n)]
    table = ReplayPolicy(cenv, traces)

    def act_fn(net, idx, f, lists, lens, masks):
        k = torch.minimum(cenv.steps_taken, table.lens)
        return table.table[torch.arange(n), k][idx.cpu()].to(f.device)
    orders = np.stack([g[f"g{i}_order"].astype(np.int64) for i in range(n)])
    res = evaluation.run_evaluation_episodes(cenv, [object(), object(), object(), object()], orders, act_fn=act_fn)
    for i in range(n):
        w, vp, steps, dec = [int(x) for x in g[f"g{i}_result"]]
        assert (int(res["winner"][i]), int(res["victory_points"][i]), int(res["game_steps"][i]), int(res["policy_decisions"][i])) == (w, vp, steps, dec), i
    blobs = env.export_state().cpu().numpy()
    for i in range(n):
        assert np.array_equal(blobs[i], g[f"g{i}_final_blob"]), spec.describe_state_diff(g[f"g{i}_final_blob"], blobs[i])
